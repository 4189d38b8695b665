"""Sample-chained prediction, the parts that need no GPU: the C-ABI declarations, the Python and
Julia bindings' shape, and a CPU check of the yardstick the GPU tests replay against
(tests/_sample_chain_ref.py)."""
import inspect
import os
import re

import numpy as np

from oracle import gpar_oracle as O
from _sample_chain_ref import _ref_samples

import gparatscale as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gpar_hip.h")).read()
SHIM = open(os.path.join(ROOT, "julia", "GPARatScaleHIP.jl")).read()

ARGS = ["n_star", "t_star", "v_shared", "ldvs", "d_shared", "v_samp", "ld_s", "ld_r", "samples",
        "seed", "f_out", "ldf_s", "ldf_r", "mean", "std"]


def _proto(name):
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, code, re.S)
    assert m, f"{name} is not declared in include/gpar_hip.h"
    return [re.match(r".*?(\w+)$", " ".join(a.split())).group(1) for a in m.group(1).split(",")]


def test_header_declares_both_entry_points_and_keeps_abi_1():
    assert _proto("gpar_predict_samples") == ["ctx", "prob", "theta"] + ARGS
    assert _proto("gpar_posterior_predict_samples") == ["ctx", "post", "i"] + ARGS
    assert re.search(r"#define GPAR_ABI_VERSION 1\b", HEADER)
    # the in-place chain is documented where the prototype is
    assert "f_out may point into the tensor v_samp points into" in HEADER


def test_exported_names_both_entry_points():
    assert "gpar_predict_samples" in G.EXPORTED
    assert "gpar_posterior_predict_samples" in G.EXPORTED


def _params(f):
    return list(inspect.signature(f).parameters)


def test_python_signatures():
    p = _params(G.predict_samples_scaled)
    assert p[:11] == ["input_locations", "pseudo_input_locations", "time_loc", "outputs", "theta",
                      "inference_time_loc", "shared_inputs", "sample_inputs", "samples", "seed",
                      "out"]
    sig = inspect.signature(G.predict_samples_scaled).parameters
    assert sig["samples"].default is None and sig["seed"].default == 0 and sig["out"].default is None
    assert _params(G.Posterior.predict_samples) == ["self", "i", "t_star", "shared_inputs",
                                                    "sample_inputs", "samples", "seed", "out"]
    sig = inspect.signature(G.Posterior.predict_samples).parameters
    assert sig["samples"].default is None and sig["seed"].default == 0 and sig["out"].default is None
    assert _params(G.Posterior.sample_chain) == ["self", "t_star", "given_inputs", "samples", "seed"]
    assert inspect.signature(G.Posterior.sample_chain).parameters["seed"].default == 0


def test_julia_shim_exports_one_host_ccall():
    src = re.sub(r"#=.*?=#", "", SHIM, flags=re.S)
    export = re.search(r"export ([\w,\s]+)\n", src).group(1)
    assert "get_gpar_scaled_prediction_samples" in export
    m = re.search(r"^function get_gpar_scaled_prediction_samples\((.*?)\)\n(.*?)\nend\n", src,
                  re.S | re.M)
    assert m, "function missing"
    pos, _, kw = m.group(1).partition(";")
    names = lambda s: re.findall(r"(?:^|,)\s*(\w+)", re.sub(r"=[^,]*", "", s))
    assert names(pos) == ["input_locations", "pseudo_input_locations", "time_loc", "outputs",
                          "theta", "inference_time_loc", "shared_inference_inputs",
                          "sample_inference_inputs"]
    for k in ("samples", "seed", "out_kernel_structure", "time_kernel_structure"):
        assert re.search(r"\b%s\b" % k, kw), k
    body = m.group(2)
    assert body.count("ccall(") == 1
    assert body.count("ccall((:gpar_predict_samples, libgpar), Int32,") == 1
    assert "GPAR_MEM_HOST" in body
    assert "return F, means, stds" in body


def _case(S, seed=0):
    t, Y = O.synthetic_gpar(140, 3, seed=5, noise=0.3)
    V = np.ascontiguousarray(Y[:, :2].T)
    Z = O.pick_pseudo_inputs(V, 12, 3)
    y = Y[:, 2].copy()
    rng = np.random.default_rng(seed)
    ts = rng.uniform(t[0], t[-1], 31)                      # unsorted test times
    Vs = np.vstack([np.interp(ts, t, V[q]) for q in range(2)])
    xi_u = rng.standard_normal((Z.shape[1], S))
    xi_p = rng.standard_normal((S, len(t) + len(ts), 4))
    return V, Z, t, y, ts, Vs, xi_u, xi_p


def test_yardstick_with_equal_inputs_is_the_path_estimator():
    """Every sample's inputs equal one V*: _ref_samples is get_gpar_scaled_predictions_path_fixed,
    however the columns are split between shared and per-sample."""
    S = 7
    V, Z, t, y, ts, Vs, xi_u, xi_p = _case(S)
    theta = (1.3, 0.9, 0.8, 1.1, 0.2)
    rm, rs = O.get_gpar_scaled_predictions_path_fixed(V, Z, t, y, ts, Vs, theta, xi_u, xi_p)
    rep = np.repeat(Vs.T[None], S, axis=0)                 # S x N* x 2
    for d_sh in (2, 1, 0):
        shared = Vs[:d_sh] if d_sh else None
        samp = rep[:, :, d_sh:] if d_sh < 2 else None
        F, mean, std = _ref_samples(V, Z, t, y, ts, shared, samp, theta, xi_u, xi_p)
        assert F.shape == (S, len(ts))
        np.testing.assert_allclose(mean, rm, rtol=1e-12, atol=1e-12 * np.abs(rm).max())
        np.testing.assert_allclose(std, rs, rtol=1e-12, atol=1e-12 * np.abs(rs).max())
        np.testing.assert_allclose(F.mean(0), mean, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(F.std(0, ddof=1), std, rtol=1e-12, atol=1e-14)


def test_yardstick_samples_see_only_their_own_inputs():
    S = 4
    V, Z, t, y, ts, Vs, xi_u, xi_p = _case(S, seed=2)
    theta = (1.3, 0.9, 0.8, 1.1, 0.2)
    rng = np.random.default_rng(9)
    samp = np.repeat(Vs.T[None, :, 1:], S, axis=0) + 0.1 * rng.standard_normal((S, len(ts), 1))
    F0, _, _ = _ref_samples(V, Z, t, y, ts, Vs[:1], samp, theta, xi_u, xi_p)
    samp2 = samp.copy()
    samp2[2] += 0.3
    F1, _, _ = _ref_samples(V, Z, t, y, ts, Vs[:1], samp2, theta, xi_u, xi_p)
    keep = [0, 1, 3]
    assert np.array_equal(F0[keep], F1[keep])
    assert np.abs(F0[2] - F1[2]).max() > 1e-6
