"""score_samples' / score_gaussian's Python-side validation and their bindings (no GPU).

Everything the C side cannot see -- the tensors' types, dtypes and ranks, the shape of y against the
predictions, the sign of the strides, levels or bins that are not numbers -- raises DomainError
before a context is asked for, so it is checked here with `context` replaced by a function that
fails the test.  The header must declare gpar_score_samples and gpar_score_gaussian, and _lib.py
must bind them with the ctypes equivalents of their prototypes."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

G = pytest.importorskip("gparatscale")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gpar_hip.h")).read()


@pytest.fixture
def no_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(G.api, "context", boom)
    monkeypatch.setattr(G.api._lib, "load", boom)


F3 = np.random.default_rng(0).standard_normal((5, 7, 3))
Y2 = F3[0] + 0.1
M2 = F3[1]
S2 = np.abs(F3[2]) + 0.1


@pytest.mark.parametrize("F", [
    F3.astype(np.float32),                 # dtype
    F3.astype(np.int64),
    F3[0, 0],                              # rank 1
    F3[None],                              # rank 4
    F3.tolist(),                           # not an array
    F3[:0],                                # no samples
    F3[:, :0],                             # no points
    F3[::-1],                              # a negative stride
    np.broadcast_to(F3[:1], (4, 7, 3)),    # a zero stride
], ids=["float32", "int64", "rank1", "rank4", "list", "S=0", "n=0", "negative", "broadcast"])
def test_bad_samples_raise_before_the_library(no_library_call, F):
    with pytest.raises(G.DomainError):
        G.score_samples(F, Y2)


@pytest.mark.parametrize("y", [
    Y2[:, :2],                             # P
    Y2[:6],                                # N*
    Y2.T.copy(),                           # transposed shape
    Y2[:, 0],                              # rank
    Y2.astype(np.float32),
    Y2.tolist(),
    Y2[::-1],                              # a negative stride
    np.broadcast_to(Y2[:1], (7, 3)),       # a zero stride
    F3,                                    # the samples' own shape
], ids=["P", "n", "transposed", "rank", "float32", "list", "negative", "broadcast", "rank3"])
def test_bad_targets_raise_before_the_library(no_library_call, y):
    with pytest.raises(G.DomainError):
        G.score_samples(F3, y)
    with pytest.raises(G.DomainError):
        G.score_gaussian(M2, S2, y)


def test_rank_two_samples_want_rank_one_targets(no_library_call):
    with pytest.raises(G.DomainError):
        G.score_samples(F3[:, :, 0], Y2)
    with pytest.raises(G.DomainError):
        G.score_gaussian(M2[:, 0], S2[:, 0], Y2)


@pytest.mark.parametrize("mean,std", [
    (M2.astype(np.float32), S2), (M2, S2.astype(np.float32)), (M2.tolist(), S2), (M2, S2.tolist()),
    (M2, S2[:, :2]), (M2[None], S2), (M2[:0], S2[:0]), (M2[::-1], S2), (M2, S2[:, ::-1]),
    (np.float64(1.0), np.float64(1.0)),
], ids=["mean32", "std32", "mean list", "std list", "std shape", "rank3", "empty", "mean negative",
        "std negative", "scalars"])
def test_bad_gaussian_predictions_raise_before_the_library(no_library_call, mean, std):
    with pytest.raises(G.DomainError):
        G.score_gaussian(mean, std, Y2)


@pytest.mark.parametrize("levels", [(), ("a",), None, (0.5, "b")],
                         ids=["empty", "text", "none", "one text"])
def test_levels_that_are_not_numbers_raise_before_the_library(no_library_call, levels):
    with pytest.raises(G.DomainError):
        G.score_samples(F3, Y2, levels=levels)
    with pytest.raises(G.DomainError):
        G.score_gaussian(M2, S2, Y2, levels=levels)


@pytest.mark.parametrize("bins", [2.5, "10", None, True], ids=["float", "text", "none", "bool"])
def test_bins_that_are_not_integers_raise_before_the_library(no_library_call, bins):
    with pytest.raises(G.DomainError):
        G.score_samples(F3, Y2, bins=bins)
    with pytest.raises(G.DomainError):
        G.score_gaussian(M2, S2, Y2, bins=bins)


def test_domain_error_is_a_value_error(no_library_call):
    with pytest.raises(ValueError):
        G.score_samples(F3, Y2[:, :1])


def test_signatures():
    p = inspect.signature(G.score_samples).parameters
    assert list(p) == ["F", "y", "levels", "bins", "entries", "device"]
    assert (p["levels"].default, p["bins"].default, p["entries"].default,
            p["device"].default) == ((0.5, 0.9, 0.95), 10, False, 0)
    p = inspect.signature(G.score_gaussian).parameters
    assert list(p) == ["mean", "std", "y", "levels", "bins", "entries", "device"]
    assert (p["levels"].default, p["bins"].default, p["entries"].default,
            p["device"].default) == ((0.5, 0.9, 0.95), 10, False, 0)
    p = inspect.signature(G.Posterior.sample_chain_scores).parameters
    assert list(p) == ["self", "t_star", "given_inputs", "samples", "y_star", "levels", "bins",
                       "seed"]
    assert (p["levels"].default, p["bins"].default, p["seed"].default) == ((0.5, 0.9, 0.95), 10, 0)


def test_result_fields():
    names = [f.name for f in dataclasses.fields(G.SampleScores)]
    assert names == ["crps", "coverage", "pit_hist", "scored", "missing", "bad", "levels",
                     "crps_entries", "below", "equal"]
    names = [f.name for f in dataclasses.fields(G.GaussianScores)]
    assert names[:9] == ["crps", "log_density", "mse", "coverage", "pit_hist", "scored", "missing",
                         "bad", "levels"]


C_TO_CTYPES = {"gpar_ctx*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64,
               "const double*": C.c_void_p, "double*": C.c_void_p, "int32_t*": C.c_void_p,
               "int64_t*": C.c_void_p}

def PLANE(t, a):
    return [(t, a[0]), ("int64_t", a[1]), ("int64_t", a[2])]


AGG = [("int64_t*", "pit_hist"), ("int64_t*", "scored"), ("int64_t*", "missing"),
       ("int64_t*", "bad")]
OPTS = [("int32_t", "nlevels"), ("const double*", "levels"), ("int32_t", "bins"),
        ("int32_t", "mem")]
EXPECTED = {
    "gpar_score_samples":
        [("gpar_ctx*", "ctx"), ("int32_t", "samples"), ("int64_t", "n"), ("int64_t", "p"),
         ("const double*", "f"), ("int64_t", "ld_s"), ("int64_t", "ld_r"), ("int64_t", "ld_c")]
        + PLANE("const double*", ("y", "ldy_r", "ldy_c")) + OPTS
        + PLANE("double*", ("crps_e", "ldc_r", "ldc_c"))
        + PLANE("int32_t*", ("below_e", "ldb_r", "ldb_c"))
        + PLANE("int32_t*", ("equal_e", "lde_r", "lde_c"))
        + [("double*", "crps"), ("double*", "coverage")] + AGG,
    "gpar_score_gaussian":
        [("gpar_ctx*", "ctx"), ("int64_t", "n"), ("int64_t", "p")]
        + PLANE("const double*", ("mean", "ldm_r", "ldm_c"))
        + PLANE("const double*", ("std", "lds_r", "lds_c"))
        + PLANE("const double*", ("y", "ldy_r", "ldy_c")) + OPTS
        + PLANE("double*", ("crps_e", "ldc_r", "ldc_c"))
        + PLANE("double*", ("logdens_e", "ldl_r", "ldl_c"))
        + PLANE("double*", ("sqerr_e", "ldq_r", "ldq_c"))
        + [("double*", "crps"), ("double*", "log_density"), ("double*", "mse"),
           ("double*", "coverage")] + AGG,
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_declares_and_lib_binds_the_entry_point(name):
    src = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, f"include/gpar_hip.h does not declare {name}"
    params = []
    for a in m.group(1).split(","):
        typ, pname = re.match(r"(.*?)\s*(\w+)$", " ".join(a.split())).groups()
        params.append((typ.replace(" *", "*"), pname))
    assert params == EXPECTED[name]
    assert re.search(r"#define GPAR_ABI_VERSION 1\b", HEADER)   # the change only adds
    assert name in G.EXPORTED
    f = getattr(G.load(), name)
    assert f.restype is C.c_int32
    assert list(f.argtypes) == [C_TO_CTYPES[t] for t, _ in params]


def test_counters_are_known_names():
    assert G.debug_counter("score_reg") >= 0 and G.debug_counter("score_lds") >= 0
    assert G.debug_counter("score_nope") == -1
