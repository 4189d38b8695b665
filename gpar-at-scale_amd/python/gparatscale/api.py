"""Python mirror of the reference's Julia API for the hot path (same names, argument
meaning and error behaviour), on top of the C-ABI in include/gpar_hip.h.

Reference functions mirrored (TudorParas/GPAR-at-scale):
  compute_gpar_dtc_objective     src/gp/dtc.jl:83-128
  get_optim_scaled_gpar_params   src/gp/dtc.jl:11-77
  compute_q_u                    src/gp/gpar_scaled_inference.jl:141-196
  get_gpar_scaled_predictions    src/gp/gpar_scaled_inference.jl:20-136
  create_lgssm / logpdf          src/gp/temporal_gp_inference.jl:15-39, :286-296
  get_sde_predictions            src/gp/temporal_gp_inference.jl:45-114
  create_optim_gp[_post] / create_optim_gpar[_post] logpdf / marginals  src/gp/optimized.jl

Inputs follow the reference's conventions: V / Z are ColVecs-like D x N matrices (or a list of
D length-N vectors, util.jl:16-31); theta in natural units (unpack_gpar, util.jl:45-55);
initial values are log-params (i_log_*), missing ones drawn U(0,1) like util.jl:128-134.
Host numpy arrays go through GPAR_MEM_HOST; torch CUDA tensors (rows = points) through
GPAR_MEM_DEVICE without host copies.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import GparFitOptions, GparProblem, KERNEL_ID, context

DEFAULT_TIME_LIMIT = 1000.0  # dtc.jl:21


# ----------------------------------------------------------------------------- util.jl
def unpack_gp(params):
    """util.jl:36-43."""
    return tuple(float(np.exp(p) + 1e-3) for p in list(params)[:3])


def unpack_gpar(params):
    """util.jl:45-55."""
    return tuple(float(np.exp(p) + 1e-3) for p in list(params)[:5])


def get_time_mask(input_length):
    """util.jl:102-106."""
    m = np.zeros(input_length)
    m[0] = 1.0
    return m


def get_output_mask(input_length):
    """util.jl:111-123; DomainError for input_length <= 1."""
    if input_length <= 1:
        raise _lib.DomainError(_lib.GPAR_ERR_ARG, "Input length must be integer greater than 1")
    m = np.zeros((input_length - 1, input_length))
    for r in range(input_length - 1):
        m[r, r + 1] = 1.0
    return m


def parse_initial_params(vals, rng=None):
    """util.jl:141-169: missing initial log-params are U(0,1) draws."""
    rng = rng if rng is not None else np.random.default_rng()
    return np.array([rng.random() if v is None else float(v) for v in vals], dtype=np.float64)


def parse_initial_gp_params(i_log_l, i_log_process_var, i_log_noise_sigma, rng=None):
    """util.jl:141-147."""
    return parse_initial_params([i_log_l, i_log_process_var, i_log_noise_sigma], rng)


def parse_initial_gpar_params(i_log_time_l, i_log_time_var, i_log_out_l, i_log_out_var,
                              i_log_noise_sigma, rng=None):
    """util.jl:154-169."""
    return parse_initial_params([i_log_time_l, i_log_time_var, i_log_out_l, i_log_out_var,
                                 i_log_noise_sigma], rng)


def to_colvecs(inputs):
    """util.jl:16-31: list of per-dimension vectors -> D x N."""
    if _is_torch(inputs):
        return inputs
    if isinstance(inputs, np.ndarray):
        return np.atleast_2d(np.asarray(inputs, dtype=np.float64))
    return np.vstack([np.asarray(a, dtype=np.float64) for a in inputs])


# ----------------------------------------------------------------------------- marshalling
def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _kernel_id(k):
    if isinstance(k, int):
        return k
    return KERNEL_ID[str(k).lower()]


class _Keep(list):
    pass


def _host_vec(x, keep):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    keep.append(a)
    return a.ctypes.data


def _host_points(X, keep):
    """D x N (ColVecs) -> point-major N x D contiguous; returns (ptr, ld, n, d)."""
    X = to_colvecs(X)
    P = np.ascontiguousarray(X.T)
    keep.append(P)
    return P.ctypes.data, P.shape[1], P.shape[0], P.shape[1]


def _dev_points(X, keep):
    """torch CUDA tensor with rows = points (N x D, unit column stride)."""
    if X.dim() == 1:
        X = X.reshape(-1, 1)
    assert X.dtype.is_floating_point and X.element_size() == 8, "float64 tensors required"
    if X.stride(1) != 1:
        X = X.contiguous()
    keep.append(X)
    return X.data_ptr(), X.stride(0), X.shape[0], X.shape[1]


def _dev_vec(x, keep):
    x = x.contiguous()
    keep.append(x)
    return x.data_ptr()


@contextlib.contextmanager
def _after_torch(ctx, on=True):
    """Device inputs are produced on torch's current stream (a .contiguous() copy above may still
    be in flight): for the calls inside the block the library's streams wait for it, device side,
    before their kernels.  The stream is forgotten again on exit, so no later call (host-memory
    ones included) touches a handle torch may since have freed."""
    if not on:
        yield
        return
    import torch
    ctx.follow_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    try:
        yield
    finally:
        ctx.follow_stream(0, enable=False)


_MODES = {"analytic": _lib.GPAR_PREDICT_ANALYTIC, "mc": _lib.GPAR_PREDICT_MC,
          "path": _lib.GPAR_PREDICT_PATH}


def _mode_id(mode):
    """Prediction mode: "analytic" (the MC estimator's S -> infinity limit), "mc" (the reference's
    estimator, gpar_scaled_inference.jl:110-130) or "path" (tmp.jl:119-167: posterior_rand paths)."""
    if mode not in _MODES:
        raise _arg_error(f"mode must be one of {sorted(_MODES)}")
    return _MODES[mode]


def _arg_error(msg):
    return _lib.DomainError(_lib.GPAR_ERR_ARG, msg)


def make_problem(V, Z, t, y, out_kernel="matern52", time_kernel="matern52", kuu_noise=True,
                 keep=None, qu_kuu_noise=False):
    """Build a gpar_problem.  Host: V, Z as D x N / D x M (ColVecs).  Device: torch tensors
    with rows = points (N x D, M x D)."""
    keep = keep if keep is not None else _Keep()
    p = GparProblem()
    dev = _is_torch(t)
    if dev:
        p.v, p.ldv, n, d = _dev_points(V, keep)
        p.z, p.ldz, m, dz = _dev_points(Z, keep)
        p.t = _dev_vec(t, keep)
        p.y = _dev_vec(y, keep)
        p.mem = _lib.GPAR_MEM_DEVICE
        # the C side cannot see device buffer lengths: check them here
        if t.numel() != n or y.numel() != n:
            raise _arg_error("t, y and V must have the same length")
    else:
        p.v, p.ldv, n, d = _host_points(V, keep)
        p.z, p.ldz, m, dz = _host_points(Z, keep)
        p.t = _host_vec(t, keep)
        p.y = _host_vec(y, keep)
        p.mem = _lib.GPAR_MEM_HOST
        if len(np.asarray(t)) != n or len(np.asarray(y)) != n:
            raise _arg_error("t, y and V must have the same length")
    if d != dz:
        raise _lib.DomainError(_lib.GPAR_ERR_ARG, "V and Z must have the same dimension")
    p.n, p.m, p.d = n, m, d
    p.out_kernel = _kernel_id(out_kernel)
    p.time_kernel = _kernel_id(time_kernel)
    p.kuu_noise = 1 if kuu_noise else 0
    p.qu_kuu_noise = 1 if qu_kuu_noise else 0
    return p, keep


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ----------------------------------------------------------------------------- DTC objective
def compute_gpar_dtc_objective(V, Z, t, y, theta, out_kernel="matern52", time_kernel="matern52",
                               kuu_noise=True, return_A=False, device=0):
    """dtc.jl:83-128.  theta = (time_l, time_var, out_l, out_var, noise_sigma), natural units.

    Returns the DTC log marginal likelihood; with return_A=True returns (dtc, A) like the
    reference (A = chol(cov(u)).U' \\ beta', M x N)."""
    ctx = context(device)
    lib = _lib.load()
    p, keep = make_problem(V, Z, t, y, out_kernel, time_kernel, kuu_noise)
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(5))
    out = np.zeros(1)
    with _after_torch(ctx, p.mem == _lib.GPAR_MEM_DEVICE):
        if return_A:
            A = np.zeros((p.n, p.m))  # column-major M x N == row-major N x M
            ctx.check(lib.gpar_dtc_objective_A(ctx.h, C.byref(p), _ptr(th), _ptr(out), _ptr(A)))
            return float(out[0]), A.T.copy()
        ctx.check(lib.gpar_dtc_objective(ctx.h, C.byref(p), 1, _ptr(th), _ptr(out)))
    return float(out[0])


def dtc_objective_batch(problems, thetas, device=0):
    """Batched objective over independent outputs (one GPU round)."""
    ctx = context(device)
    lib = _lib.load()
    arr = (GparProblem * len(problems))(*problems)
    th = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64).reshape(len(problems), 5))
    out = np.zeros(len(problems))
    with _after_torch(ctx, problems[0].mem == _lib.GPAR_MEM_DEVICE):
        ctx.check(lib.gpar_dtc_objective(ctx.h, arr, len(problems), _ptr(th), _ptr(out)))
    return out


def pairwise_distances(V, Z, out_kernel="matern52", device=0):
    """The distances Kfu = pairwise(k_o, V, Z) is built from (dtc.jl:104), as the fit's distance
    cache holds them (gpar_pairwise_distances): |v_k - z_c| for the Matern kernels, squared for
    EQ; N x M.  Host V / Z (D x N / D x M ColVecs) or device tensors (rows = points)."""
    ctx, lib = context(device), _lib.load()
    if _is_torch(V):
        import torch
        n = V.shape[0]
        t = torch.arange(n, dtype=torch.float64, device=V.device)
        p, keep = make_problem(V, Z, t, torch.zeros_like(t), out_kernel)
        out = torch.empty((n, p.m), dtype=torch.float64, device=V.device)
        with _after_torch(ctx):
            ctx.check(lib.gpar_pairwise_distances(ctx.h, C.byref(p), C.c_void_p(out.data_ptr())))
        return out
    n = to_colvecs(V).shape[1]
    p, keep = make_problem(V, Z, np.arange(n, dtype=np.float64), np.zeros(n), out_kernel)
    out = np.zeros((n, p.m))
    ctx.check(lib.gpar_pairwise_distances(ctx.h, C.byref(p), _ptr(out)))
    return out


# ----------------------------------------------------------------------------- pseudo-input selection
@dataclass
class PseudoInputs:
    """select_pseudo_inputs' result.  Z: the centres, laid out as the inputs were (host: D x M
    ColVecs, device: M x D tensor), ready to pass on as pseudo_input_locations; index: [M] the row
    of V each centre was snapped to (-1: empty cluster, or snap=False); labels: [N] each input's
    centre; counts: [M] members per centre; inertia: [iters + 1] host array, the sum of squared
    distances of every assignment pass (labels / counts / inertia[-1] refer to the centres before
    the snap)."""
    Z: object
    index: object
    labels: object
    counts: object
    inertia: np.ndarray


def select_pseudo_inputs(V, Z0_or_M, iters=10, snap=True, seed=0, device=0):
    """Place M pseudo-inputs over the inputs V by Lloyd's k-means on the GPU
    (gpar_select_pseudo_inputs): `iters` rounds from the start centres, then with snap=True every
    non-empty cluster's centre is replaced by its member row nearest to it, so Z is M distinct rows
    of V.  V: host D x N (ColVecs) or a device tensor N x D (rows = points; a column-prefix view of
    a wider matrix is read in place).  Z0_or_M: the start centres, laid out like V, or an integer
    M: the rows data.pseudo_index(N, M, seed) of V.  Deterministic."""
    from . import data
    ctx, lib = context(device), _lib.load()
    keep = _Keep()
    dev = _is_torch(V)
    if dev:
        import torch
        vp, ldv, n, d = _dev_points(V, keep)
        Vr = keep[-1]
        if isinstance(Z0_or_M, (int, np.integer)):
            if not 1 <= int(Z0_or_M) <= n:
                raise _arg_error("M must be in 1..N")
            rows = torch.as_tensor(data.pseudo_index(n, int(Z0_or_M), seed), device=Vr.device)
            Z0 = Vr[rows]
        else:
            Z0 = Z0_or_M
        zp, ldz, m, dz = _dev_points(Z0, keep)
        if dz != d:
            raise _arg_error("V and Z0 must have the same dimension")
        opt = dict(device=Vr.device)
        Z = torch.empty((m, d), dtype=torch.float64, **opt)
        index = torch.empty(m, dtype=torch.int64, **opt)
        labels = torch.empty(n, dtype=torch.int32, **opt)
        counts = torch.empty(m, dtype=torch.int64, **opt)
        ptr = lambda a: C.c_void_p(a.data_ptr())
        mem = _lib.GPAR_MEM_DEVICE
    else:
        vp, ldv, n, d = _host_points(V, keep)
        Vr = keep[-1]
        if isinstance(Z0_or_M, (int, np.integer)):
            if not 1 <= int(Z0_or_M) <= n:
                raise _arg_error("M must be in 1..N")
            Z0 = Vr[data.pseudo_index(n, int(Z0_or_M), seed)].T
        else:
            Z0 = Z0_or_M
        zp, ldz, m, dz = _host_points(Z0, keep)
        if dz != d:
            raise _arg_error("V and Z0 must have the same dimension")
        Z = np.zeros((m, d))
        index = np.zeros(m, dtype=np.int64)
        labels = np.zeros(n, dtype=np.int32)
        counts = np.zeros(m, dtype=np.int64)
        ptr = _ptr
        mem = _lib.GPAR_MEM_HOST
    inertia = np.zeros(max(int(iters), 0) + 1)
    with _after_torch(ctx, dev):
        ctx.check(lib.gpar_select_pseudo_inputs(
            ctx.h, n, d, C.c_void_p(vp), ldv, m, C.c_void_p(zp), ldz, int(iters),
            1 if snap else 0, mem, ptr(Z), d, ptr(index), ptr(labels), ptr(counts),
            _ptr(inertia)))
    return PseudoInputs(Z if dev else np.ascontiguousarray(Z.T), index, labels, counts, inertia)


# ----------------------------------------------------------------------------- fit
@dataclass
class FitResult:
    theta: np.ndarray      # P x 5 natural units
    nlml: np.ndarray       # P
    evals: np.ndarray      # P


def fit_batch(problems, log_theta0, max_evals=0, max_iterations=1000, g_tol=1e-8,
              time_limit=0.0, device=0):
    """Batched NelderMead over outputs (gpar_fit)."""
    ctx = context(device)
    lib = _lib.load()
    P = len(problems)
    arr = (GparProblem * P)(*problems)
    x0 = np.ascontiguousarray(np.asarray(log_theta0, dtype=np.float64).reshape(P, 5))
    opts = GparFitOptions(int(max_evals), int(max_iterations), float(g_tol), float(time_limit))
    theta = np.zeros((P, 5))
    nlml = np.zeros(P)
    evals = np.zeros(P, dtype=np.int32)
    with _after_torch(ctx, problems[0].mem == _lib.GPAR_MEM_DEVICE):
        ctx.check(lib.gpar_fit(ctx.h, arr, P, _ptr(x0), C.byref(opts), _ptr(theta), _ptr(nlml),
                               _ptr(evals)))
    return FitResult(theta, nlml, evals)


def fit_predict_batch(problems, log_theta0, t_star, V_stars, max_evals=0, max_iterations=1000,
                      g_tol=1e-8, time_limit=0.0, mode="analytic", samples=100, seed=0, device=0,
                      keep=None, chain=None, chain_cols=None):
    """get_gpar_scaled_predictions (gpar_scaled_inference.jl:20-136) for a batch of outputs
    (gpar_fit_predict): the batched fit, then each output's prediction at its fitted theta,
    reusing the fit's Gram at that theta for q(u) when the problem has qu_kuu_noise.

    Device problems (make_problem on torch tensors): t_star a device vector, V_stars[i] output
    i's test inputs (N* x D_i tensor, rows = points); returns (FitResult, means, stds) with
    means/stds lists of device tensors.  Host problems: numpy t_star and D_i x N* ColVecs.

    Chained inference inputs (gpar_fit_predict_chain; GPAR_scaled_examples.jl:172 feeds y2's
    predicted means to y3): `chain` is an N* x K matrix (numpy C-order array for host problems, a
    device tensor with unit column stride otherwise), `chain_cols[i]` the column output i's
    predicted mean is written to after its prediction (-1: none).  V_stars[i] = None reads output
    i's inputs from chain's first D_i columns, as they stand when its prediction runs (columns of
    earlier outputs hold their predicted means, the others what the caller put there)."""
    P = len(problems)
    keep = keep if keep is not None else _Keep()
    if chain is not None:
        if chain_cols is None or len(chain_cols) != P:
            raise _arg_error("chain_cols needs one entry per problem")
        K = chain.shape[1]
        if any(c >= K for c in chain_cols):
            raise _arg_error("chain_cols entries must be < chain.shape[1]")
        if _is_torch(chain):
            if chain.stride(1) != 1 or chain.dtype != __import__("torch").float64:
                raise _arg_error("chain must be a float64 tensor with unit column stride")
            chain_ptr, ld_chain = chain.data_ptr(), chain.stride(0)
        else:
            if not (isinstance(chain, np.ndarray) and chain.dtype == np.float64 and chain.flags.c_contiguous):
                raise _arg_error("chain must be a C-contiguous float64 numpy array")
            chain_ptr, ld_chain = chain.ctypes.data, K
    elif any(v is None for v in V_stars):
        raise _arg_error("V_stars[i] = None needs a chain")
    arr = (GparProblem * P)(*problems)
    x0 = np.ascontiguousarray(np.asarray(log_theta0, dtype=np.float64).reshape(P, 5))
    opts = GparFitOptions(int(max_evals), int(max_iterations), float(g_tol), float(time_limit))
    theta = np.zeros((P, 5))
    nlml = np.zeros(P)
    evals = np.zeros(P, dtype=np.int32)
    dev = problems[0].mem == _lib.GPAR_MEM_DEVICE
    vptr, ldvs, means, stds = [], [], [], []
    if len(V_stars) != P:
        raise _arg_error("one V_star per problem")
    n_star = t_star.numel() if dev else len(np.asarray(t_star))
    if dev:
        import torch
        tsp = _dev_vec(t_star, keep)
        for i, Vs in enumerate(V_stars):
            if Vs is None:
                Vs = chain[:, : problems[i].d]
            p_, ld_, ns, ds = _dev_points(Vs, keep)
            if ns != n_star or ds != problems[i].d:
                raise _arg_error(f"V_stars[{i}] must be N* x D = {n_star} x {problems[i].d}")
            vptr.append(p_)
            ldvs.append(ld_)
            means.append(torch.empty(ns, dtype=torch.float64, device=t_star.device))
            stds.append(torch.empty(ns, dtype=torch.float64, device=t_star.device))
        mp_ = [m.data_ptr() for m in means]
        sp_ = [x.data_ptr() for x in stds]
    else:
        tsp = _host_vec(t_star, keep)
        for i, Vs in enumerate(V_stars):
            if Vs is None:   # read in place from the chain (aliasing is the point)
                if problems[i].d > chain.shape[1] or chain.shape[0] != n_star:
                    raise _arg_error(f"chain must be N* x K with K >= D_{i}")
                p_, ld_, ns, ds = chain.ctypes.data, chain.shape[1], chain.shape[0], problems[i].d
            else:
                p_, ld_, ns, ds = _host_points(Vs, keep)
            if ns != n_star or ds != problems[i].d:
                raise _arg_error(f"V_stars[{i}] must be D x N* = {problems[i].d} x {n_star}")
            vptr.append(p_)
            ldvs.append(ld_)
            means.append(np.zeros(ns))
            stds.append(np.zeros(ns))
        mp_ = [m.ctypes.data for m in means]
        sp_ = [x.ctypes.data for x in stds]
    ns = n_star
    ctx, lib = context(device), _lib.load()
    VP = (C.c_void_p * P)(*vptr)
    LD = (C.c_int64 * P)(*ldvs)
    MP = (C.c_void_p * P)(*mp_)
    SP = (C.c_void_p * P)(*sp_)
    md = _mode_id(mode)
    if chain is not None and dev and chain.shape[0] != n_star:
        raise _arg_error("chain must have N* rows")
    with _after_torch(ctx, dev):
        if chain is None:
            ctx.check(lib.gpar_fit_predict(ctx.h, arr, P, _ptr(x0), C.byref(opts), ns, tsp, VP, LD,
                                           md, int(samples), int(seed), _ptr(theta), _ptr(nlml),
                                           _ptr(evals), MP, SP))
        else:
            CC = (C.c_int32 * P)(*[int(c) for c in chain_cols])
            ctx.check(lib.gpar_fit_predict_chain(ctx.h, arr, P, _ptr(x0), C.byref(opts), ns, tsp, VP,
                                                 LD, md, int(samples), int(seed),
                                                 C.c_void_p(chain_ptr), int(ld_chain), CC,
                                                 _ptr(theta), _ptr(nlml), _ptr(evals), MP, SP))
    return FitResult(theta, nlml, evals), means, stds


def get_gpar_scaled_predictions_batch(Y, pseudo_input_locations, time_loc, inference_time_loc, F,
                                      chained=False, log_theta0=(0.0, 0.0, 0.0, 0.0, -2.0),
                                      max_evals=0, g_tol=1e-8, time_limit=0.0, mode="analytic",
                                      samples=100, seed=0, qu_kuu_noise=False, device=0):
    """The Julia shim's matrix-form batch driver (julia/GPARatScaleHIP.jl): GPAR's per-output loop
    (GPAR_scaled_examples.jl:132-175) for outputs 2..P of the host matrix Y (N x P, column i =
    output i; output i's inputs are columns 1..i-1), ONE matrix passed for every output's inputs
    (ldv = P; the library uploads it once) and one for the inference inputs F (N* x P; output i
    reads its first i - 1 columns, given or -- chained -- F's column 1 then predicted means).
    pseudo_input_locations[i - 2]: output i's D x M pseudo-inputs.  Returns (FitResult, means,
    stds) for outputs 2..P.

    Defaults differ from the Julia method on purpose, so that a call is reproducible: here
    mode="analytic" (Julia: mode=:mc, the reference's estimator), seed=0 (Julia: rand(UInt64)), a
    fixed log_theta0 (Julia: parse_initial_gpar_params, U(0,1) draws for missing values, util.jl:
    128-134) and no time limit (Julia: optimization_time_limit=1000.0, dtc.jl:21).  Pass
    mode="mc", a seed, log_theta0 and time_limit to reproduce a Julia call."""
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64))
    F = np.ascontiguousarray(np.array(F, dtype=np.float64))   # a copy: the chain writes into it
    n, P = Y.shape
    ns = F.shape[0]
    t = np.ascontiguousarray(np.asarray(time_loc, dtype=np.float64))
    ts = np.ascontiguousarray(np.asarray(inference_time_loc, dtype=np.float64))
    if P < 2 or F.shape[1] != P or len(t) != n or len(ts) != ns:
        raise _arg_error("Y (N x P), F (N* x P), time_loc (N), inference_time_loc (N*) disagree")
    if len(pseudo_input_locations) != P - 1:
        raise _arg_error("one pseudo-input set per output 2..P")
    keep = _Keep([Y, F, t, ts])
    probs = []
    for i in range(2, P + 1):
        p = GparProblem()
        p.z, p.ldz, m, dz = _host_points(pseudo_input_locations[i - 2], keep)
        if dz != i - 1:
            raise _arg_error(f"output {i}'s pseudo-inputs must have {i - 1} rows")
        p.n, p.m, p.d = n, m, i - 1
        p.t, p.v, p.ldv = t.ctypes.data, Y.ctypes.data, P
        p.y = _host_vec(Y[:, i - 1], keep)
        p.out_kernel = p.time_kernel = KERNEL_ID["matern52"]
        p.kuu_noise, p.mem, p.qu_kuu_noise = 1, _lib.GPAR_MEM_HOST, 1 if qu_kuu_noise else 0
        probs.append(p)
    Q = P - 1
    arr = (GparProblem * Q)(*probs)
    x0 = np.ascontiguousarray(np.tile(np.asarray(log_theta0, dtype=np.float64), (Q, 1)))
    opts = GparFitOptions(int(max_evals), 1000, float(g_tol), float(time_limit))
    theta, nlml, evals = np.zeros((Q, 5)), np.zeros(Q), np.zeros(Q, dtype=np.int32)
    means = [np.zeros(ns) for _ in range(Q)]
    stds = [np.zeros(ns) for _ in range(Q)]
    VP = (C.c_void_p * Q)(*([F.ctypes.data] * Q))
    LD = (C.c_int64 * Q)(*([P] * Q))
    MP = (C.c_void_p * Q)(*[a.ctypes.data for a in means])
    SP = (C.c_void_p * Q)(*[a.ctypes.data for a in stds])
    ctx, lib = context(device), _lib.load()
    md = _mode_id(mode)
    if chained:
        CC = (C.c_int32 * Q)(*range(1, P))
        ctx.check(lib.gpar_fit_predict_chain(ctx.h, arr, Q, _ptr(x0), C.byref(opts), ns,
                                             ts.ctypes.data, VP, LD, md, int(samples), int(seed),
                                             C.c_void_p(F.ctypes.data), P, CC, _ptr(theta),
                                             _ptr(nlml), _ptr(evals), MP, SP))
    else:
        ctx.check(lib.gpar_fit_predict(ctx.h, arr, Q, _ptr(x0), C.byref(opts), ns, ts.ctypes.data,
                                       VP, LD, md, int(samples), int(seed), _ptr(theta), _ptr(nlml),
                                       _ptr(evals), MP, SP))
    return FitResult(theta, nlml, evals), means, stds


def _samples_call(call, dev, d, t_star, shared_inputs, sample_inputs, samples, seed, out, device):
    """Marshalling of gpar_predict_samples / gpar_posterior_predict_samples (their arguments after
    the problem or posterior): `call(n_star, t_star, v_shared, ldvs, d_shared, v_samp, ld_s, ld_r,
    samples, seed, f_out, ldf_s, ldf_r, mean, std)` makes the library call.  Everything the C side
    cannot see (lengths, widths, strides of tensors) is checked here.  Returns (F, mean, std)."""
    keep = _Keep()
    ctx = context(device)
    if samples is None:
        samples = sample_inputs.shape[0] if sample_inputs is not None else 100
    S = int(samples)
    if sample_inputs is not None and (len(sample_inputs.shape) != 3 or sample_inputs.shape[0] != S):
        raise _arg_error("sample_inputs must be samples x N* x d_sa")
    if dev:
        import torch
        if not _is_torch(t_star):
            raise _arg_error("device problems take device tensors")
        ns = t_star.numel()
        tsp = _dev_vec(t_star, keep)
        vshp, ldvs, d_sh = None, 0, 0
        if shared_inputs is not None and shared_inputs.numel():
            vshp, ldvs, nr, d_sh = _dev_points(shared_inputs, keep)
            if nr != ns:
                raise _arg_error("shared_inputs must be N* x d_sh with N* = len(t_star)")
        vsap, ld_s, ld_r, d_sa = None, 0, 0, 0
        if sample_inputs is not None and sample_inputs.shape[2]:
            X = sample_inputs
            if X.dtype != torch.float64:
                raise _arg_error("float64 tensors required")
            if X.stride(2) != 1:
                X = X.contiguous()
            keep.append(X)
            if X.shape[1] != ns:
                raise _arg_error("sample_inputs must be samples x N* x d_sa with N* = len(t_star)")
            vsap, ld_s, ld_r, d_sa = X.data_ptr(), X.stride(0), X.stride(1), X.shape[2]
        if sample_inputs is not None and d_sh + d_sa != d:
            raise _arg_error(f"shared ({d_sh}) and sample ({d_sa}) input columns must add up to D = {d}")
        if out is None:
            out = torch.empty((max(S, 0), ns), dtype=torch.float64, device=t_star.device)
        elif (not _is_torch(out) or out.dtype != torch.float64 or tuple(out.shape) != (S, ns)):
            raise _arg_error("out must be a float64 samples x N* device tensor (any strides)")
        mean = torch.empty(ns, dtype=torch.float64, device=t_star.device)
        std = torch.empty(ns, dtype=torch.float64, device=t_star.device)
        with _after_torch(ctx):
            ctx.check(call(ns, tsp, vshp, ldvs, d_sh, vsap, ld_s, ld_r, S, int(seed), out.data_ptr(),
                           out.stride(0) if S > 1 else max(out.stride(0), (ns - 1) * out.stride(1) + 1),
                           out.stride(1) if ns > 1 else 1, mean.data_ptr(), std.data_ptr()))
        return out, mean, std
    ns = len(np.asarray(t_star))
    tsp = _host_vec(t_star, keep)
    vshp, ldvs, d_sh = None, 0, 0
    if shared_inputs is not None and np.size(shared_inputs):
        vshp, ldvs, nr, d_sh = _host_points(shared_inputs, keep)
        if nr != ns:
            raise _arg_error("shared_inputs must be d_sh x N* with N* = len(t_star)")
    vsap, ld_s, ld_r, d_sa = None, 0, 0, 0
    if sample_inputs is not None and sample_inputs.shape[2]:
        X = sample_inputs
        # read in place when it is a float64 array with unit last stride (a column prefix of a wider
        # S x N* x K array included), else through a packed copy
        if not (isinstance(X, np.ndarray) and X.dtype == np.float64 and X.strides[2] == 8
                and X.strides[0] % 8 == 0 and X.strides[1] % 8 == 0
                and X.strides[1] >= 8 * X.shape[2]
                and X.strides[0] >= (X.shape[1] - 1) * X.strides[1] + 8 * X.shape[2]):
            X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        keep.append(X)
        if X.shape[1] != ns:
            raise _arg_error("sample_inputs must be samples x N* x d_sa with N* = len(t_star)")
        vsap, ld_s, ld_r, d_sa = X.ctypes.data, X.strides[0] // 8, X.strides[1] // 8, X.shape[2]
    if sample_inputs is not None and d_sh + d_sa != d:
        raise _arg_error(f"shared ({d_sh}) and sample ({d_sa}) input columns must add up to D = {d}")
    if out is None:
        out = np.zeros((max(S, 0), ns))
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (S, ns)
              and out.flags.writeable and out.strides[0] % 8 == 0 and out.strides[1] % 8 == 0
              and out.strides[1] > 0 and out.strides[0] > 0):
        raise _arg_error("out must be a writable float64 samples x N* array (positive strides)")
    mean, std = np.zeros(ns), np.zeros(ns)
    ldf_r = out.strides[1] // 8 if ns > 1 else 1
    ldf_s = out.strides[0] // 8 if S > 1 else max(out.strides[0] // 8, (ns - 1) * ldf_r + 1)
    ctx.check(call(ns, tsp, vshp, ldvs, d_sh, vsap, ld_s, ld_r, S, int(seed), out.ctypes.data, ldf_s,
                   ldf_r, _ptr(mean), _ptr(std)))
    return out, mean, std


def predict_samples_scaled(input_locations, pseudo_input_locations, time_loc, outputs, theta,
                           inference_time_loc, shared_inputs, sample_inputs, samples=None, seed=0,
                           out=None, out_kernel="matern52", time_kernel="matern52", device=0,
                           qu_kuu_noise=False):
    """Joint samples of one output at the inference locations when every sample has inference
    inputs of its own (gpar_predict_samples): predict_scaled's mode="path" -- a q(u) draw and a
    posterior path of the time GP per sample -- with sample s's kernel matrix taken at
    [shared_inputs | sample_inputs[s]].  GPAR's joint draws feed sample s of the earlier outputs
    into sample s of this one that way.  The draws are mode="path"'s for (samples, seed)
    (mc_normals, path_normals), so with no sample columns this is mode="path" with its samples.

    Host problems: shared_inputs d_sh x N* (ColVecs; None or empty: no shared columns),
    sample_inputs an S x N* x d_sa array (None: no sample columns).  Device problems: N* x d_sh and
    S x N* x d_sa tensors with unit last stride; a column-prefix view of a wider S x N* x K tensor
    is read in place.  d_sh + d_sa = D.  samples: S (default: sample_inputs' first dimension).
    out: an S x N* view, possibly strided, to write the samples into -- it may be a column of the
    tensor sample_inputs is a prefix of, which is how a chain of outputs is sampled in place.

    Returns (F, mean, std): F S x N* (out when given), mean and Bessel std over the samples, all at
    the inference locations in their input order (samples = 1: std is NaN)."""
    p, keep = make_problem(input_locations, pseudo_input_locations, time_loc, outputs,
                           out_kernel, time_kernel, qu_kuu_noise=qu_kuu_noise)
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(5))
    ctx, lib = context(device), _lib.load()
    call = lambda *a: lib.gpar_predict_samples(ctx.h, C.byref(p), _ptr(th), *a)
    return _samples_call(call, p.mem == _lib.GPAR_MEM_DEVICE, p.d, inference_time_loc,
                         shared_inputs, sample_inputs, samples, seed, out, device)


def sample_quantiles(F, q, out=None, device=0):
    """Quantiles over the sample axis of joint samples (gpar_sample_quantiles): the credible bands
    of a sample chain, computed in place on the device.  F: S x N* or S x N* x P float64 samples, a
    numpy array (host memory) or a torch device tensor, any positive strides -- the chain tensor
    sample_chain returns, a column chain[:, :, c] or a row block of it are read where they are.
    q: a sequence of levels in [0, 1], any order.  Returns the len(q) x N* (x P) quantiles by
    numpy's default method ("linear"), bit-identical whatever the strides or the memory kind; an
    entry with a NaN sample gives NaN.  out: an array / tensor of that shape (any positive strides)
    to write into.  S <= 4096."""
    dev = _is_torch(F)
    if not dev and not isinstance(F, np.ndarray):
        raise _arg_error("F must be a numpy array or a torch device tensor")
    if dev:
        import torch
        f64 = F.dtype == torch.float64
    else:
        f64 = F.dtype == np.float64
    if not f64:
        raise _arg_error("F must be float64")
    if len(F.shape) not in (2, 3):
        raise _arg_error("F must be S x N* or S x N* x P")
    shape = tuple(int(x) for x in F.shape)
    if min(shape) < 1:
        raise _arg_error("F must not be empty")
    try:
        qa = np.ascontiguousarray(np.asarray(q, dtype=np.float64).ravel())
    except (TypeError, ValueError):
        raise _arg_error("q must be a sequence of numbers in [0, 1]") from None
    if qa.size < 1:
        raise _arg_error("q must hold at least one level")
    if not bool(np.all((qa >= 0.0) & (qa <= 1.0))):   # a NaN fails both comparisons
        raise _arg_error("every q must be in [0, 1]")
    nq = int(qa.size)
    oshape = (nq,) + shape[1:]

    def strides(a):
        # in doubles; a dimension of one element never steps, whatever stride it carries
        if dev:
            ld = [int(x) for x in a.stride()]
        elif any(x % 8 for x in a.strides):
            raise _arg_error("strides must be multiples of 8 bytes")
        else:
            ld = [x // 8 for x in a.strides]
        return tuple(1 if m == 1 else x for x, m in zip(ld, a.shape))

    if out is not None:
        same_kind = _is_torch(out) if dev else isinstance(out, np.ndarray)
        if not same_kind or tuple(out.shape) != oshape or out.dtype != F.dtype:
            raise _arg_error(f"out must be a float64 {'tensor' if dev else 'array'} of shape {oshape}")
        if dev and out.device != F.device:
            raise _arg_error("out must live on F's device")
        if not dev and not out.flags.writeable:
            raise _arg_error("out must be writable")
    lf = strides(F)
    lo = strides(out) if out is not None else None
    if min(lf) < 1 or (lo is not None and min(lo) < 1):
        raise _arg_error("strides must be positive")
    if dev and not F.is_cuda:
        raise _arg_error("torch tensors must be device tensors (host data: numpy arrays)")
    S, n = shape[0], shape[1]
    p = shape[2] if len(shape) == 3 else 1
    ctx, lib = context(device), _lib.load()
    if out is None:
        if dev:
            import torch
            out = torch.empty(oshape, dtype=torch.float64, device=F.device)
        else:
            out = np.empty(oshape)
        lo = strides(out)
    lf3 = lf if len(shape) == 3 else lf + (1,)
    lo3 = lo if len(shape) == 3 else lo + (1,)
    fp = F.data_ptr() if dev else F.ctypes.data
    op = out.data_ptr() if dev else out.ctypes.data
    mem = _lib.GPAR_MEM_DEVICE if dev else _lib.GPAR_MEM_HOST
    with _after_torch(ctx, dev):
        ctx.check(lib.gpar_sample_quantiles(ctx.h, S, n, p, fp, lf3[0], lf3[1], lf3[2], nq, _ptr(qa),
                                            mem, op, lo3[0], lo3[1], lo3[2]))
    return out


# ----------------------------------------------------------------------------- scores
@dataclass
class SampleScores:
    """score_samples' result, per output over its scored entries (host numpy arrays): crps [P] the
    mean ensemble CRPS, coverage [L x P] the share of targets inside the central band of each
    level, pit_hist [B x P] the counts of the mid-rank PIT bins, scored / missing / bad [P] the
    entries that count, whose target is NaN, and whose samples hold a NaN.  levels: the central
    levels.  With entries=True also crps_entries, below (#samples < y) and equal (#samples == y),
    each N* (x P), numpy or torch like F; NaN / -1 at missing or bad entries."""
    crps: np.ndarray
    coverage: np.ndarray
    pit_hist: np.ndarray
    scored: np.ndarray
    missing: np.ndarray
    bad: np.ndarray
    levels: tuple
    crps_entries: object = None
    below: object = None
    equal: object = None


@dataclass
class GaussianScores:
    """score_gaussian's result: SampleScores' aggregates (crps the mean Gaussian CRPS, pit_hist
    from Phi(z)) plus log_density [P] and mse [P], the mean log predictive density and the mean
    squared error over the scored entries; bad counts NaN mean / std and std <= 0.  With
    entries=True also crps_entries, log_density_entries, sq_err_entries, each N* (x P)."""
    crps: np.ndarray
    log_density: np.ndarray
    mse: np.ndarray
    coverage: np.ndarray
    pit_hist: np.ndarray
    scored: np.ndarray
    missing: np.ndarray
    bad: np.ndarray
    levels: tuple
    crps_entries: object = None
    log_density_entries: object = None
    sq_err_entries: object = None


def _score_tensor(a, name, dev, shape, like=None):
    """A float64 tensor of `shape` of the memory kind `dev` names -> (address, strides in doubles),
    a dimension of one element carrying stride 1; DomainError otherwise."""
    kind = "torch device tensor" if dev else "numpy array"
    if (_is_torch(a) if dev else isinstance(a, np.ndarray)) is False:
        raise _arg_error(f"{name} must be a {kind}, as the predictions are")
    if dev:
        import torch
        if a.dtype != torch.float64:
            raise _arg_error(f"{name} must be float64")
        if not a.is_cuda:
            raise _arg_error("torch tensors must be device tensors (host data: numpy arrays)")
        if like is not None and a.device != like.device:
            raise _arg_error(f"{name} must live on the predictions' device")
    elif a.dtype != np.float64:
        raise _arg_error(f"{name} must be float64")
    if shape is not None and tuple(int(x) for x in a.shape) != tuple(shape):
        raise _arg_error(f"{name} must have shape {tuple(shape)}")
    if dev:
        ld = [int(x) for x in a.stride()]
    elif any(x % 8 for x in a.strides):
        raise _arg_error("strides must be multiples of 8 bytes")
    else:
        ld = [x // 8 for x in a.strides]
    ld = tuple(1 if m == 1 else x for x, m in zip(ld, a.shape))
    if ld and min(ld) < 1:
        raise _arg_error("strides must be positive")
    return (a.data_ptr() if dev else a.ctypes.data), ld


def _score_options(levels, bins):
    if levels is None:
        raise _arg_error("levels must be a sequence of numbers in (0, 1)")
    try:
        la = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).ravel())
    except (TypeError, ValueError):
        raise _arg_error("levels must be a sequence of numbers in (0, 1)") from None
    if la.size < 1:
        raise _arg_error("levels must hold at least one level")
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
        raise _arg_error("bins must be an integer")
    return la, int(bins)


def _plane2(ld, rank):
    return ld if rank == 2 else ld + (1,)


def score_samples(F, y, levels=(0.5, 0.9, 0.95), bins=10, entries=False, device=0):
    """Score joint samples against held-out targets on the device (gpar_score_samples).  F: S x N*
    or S x N* x P float64 samples, a numpy array (host memory) or a torch device tensor, any
    positive strides (read in place, as sample_quantiles reads them); y: the targets, N* or
    N* x P, of F's kind, NaN where nothing was observed.  Per output, over the entries with a
    target and no NaN sample: the mean ensemble CRPS (E|X - y| - E|X - X'| / 2), the histogram over
    `bins` bins of the mid-rank PIT (below + equal / 2) / S, and the share of targets inside the
    central band of each level l in `levels` (at most 8, each in (0, 1)) -- the closed interval
    between sample_quantiles' quantiles (1 - l) / 2 and (1 + l) / 2, flag for flag.  Every result
    is bit-identical whatever the strides, the memory kind or the kernel path.  entries=True adds
    the per-entry CRPS and ranks.  Returns SampleScores.  S <= 4096, bins <= 64."""
    dev = _is_torch(F)
    if not dev and not isinstance(F, np.ndarray):
        raise _arg_error("F must be a numpy array or a torch device tensor")
    if len(F.shape) not in (2, 3):
        raise _arg_error("F must be S x N* or S x N* x P")
    shape = tuple(int(x) for x in F.shape)
    if min(shape) < 1:
        raise _arg_error("F must not be empty")
    fp, lf = _score_tensor(F, "F", dev, None)
    yp, ly = _score_tensor(y, "y", dev, shape[1:], like=F)
    la, nb = _score_options(levels, bins)
    S, n = shape[0], shape[1]
    p = shape[2] if len(shape) == 3 else 1
    ctx, lib = context(device), _lib.load()
    ce = be = ee = None
    cp = bp = ep = None
    if entries:
        if dev:
            import torch
            ce = torch.empty(shape[1:], dtype=torch.float64, device=F.device)
            be = torch.empty(shape[1:], dtype=torch.int32, device=F.device)
            ee = torch.empty(shape[1:], dtype=torch.int32, device=F.device)
            cp, bp, ep = ce.data_ptr(), be.data_ptr(), ee.data_ptr()
        else:
            ce = np.empty(shape[1:])
            be = np.empty(shape[1:], dtype=np.int32)
            ee = np.empty(shape[1:], dtype=np.int32)
            cp, bp, ep = ce.ctypes.data, be.ctypes.data, ee.ctypes.data
    lf3 = lf if len(shape) == 3 else lf + (1,)
    ly2 = _plane2(ly, len(shape) - 1)
    crps, cov = np.empty(p), np.empty((la.size, p))
    hist = np.zeros((max(nb, 0), p), dtype=np.int64)
    cnt = [np.zeros(p, dtype=np.int64) for _ in range(3)]
    mem = _lib.GPAR_MEM_DEVICE if dev else _lib.GPAR_MEM_HOST
    with _after_torch(ctx, dev):
        ctx.check(lib.gpar_score_samples(
            ctx.h, S, n, p, fp, lf3[0], lf3[1], lf3[2], yp, ly2[0], ly2[1], int(la.size), _ptr(la),
            nb, mem, cp, p, 1, bp, p, 1, ep, p, 1, _ptr(crps), _ptr(cov), _ptr(hist),
            _ptr(cnt[0]), _ptr(cnt[1]), _ptr(cnt[2])))
    return SampleScores(crps, cov, hist, cnt[0], cnt[1], cnt[2], tuple(float(x) for x in la),
                        ce, be, ee)


def score_gaussian(mean, std, y, levels=(0.5, 0.9, 0.95), bins=10, entries=False, device=0):
    """Score Gaussian predictions against held-out targets on the device (gpar_score_gaussian):
    the analytic and MC modes' (mean, std), on the scale score_samples uses for sample chains.
    mean, std, y: N* or N* x P float64, numpy arrays or torch device tensors of one kind, any
    positive strides; y NaN where nothing was observed.  With z = (y - mean) / std, per output
    over the entries with a target, a mean, and std > 0: the mean log density, the mean CRPS
    std (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)), the mean squared error, the histogram of
    Phi(z) over `bins` bins and the share with |z| <= Phi^-1((1 + l) / 2) for each level l.  std
    is scored as given: a prediction of the latent f scores noisy observations with
    sqrt(std**2 + sigma_n**2).  Returns GaussianScores."""
    dev = _is_torch(mean)
    if not dev and not isinstance(mean, np.ndarray):
        raise _arg_error("mean must be a numpy array or a torch device tensor")
    if len(mean.shape) not in (1, 2):
        raise _arg_error("mean must be N* or N* x P")
    shape = tuple(int(x) for x in mean.shape)
    if min(shape) < 1:
        raise _arg_error("mean must not be empty")
    mp_, lm = _score_tensor(mean, "mean", dev, None)
    sp, ls = _score_tensor(std, "std", dev, shape, like=mean)
    yp, ly = _score_tensor(y, "y", dev, shape, like=mean)
    la, nb = _score_options(levels, bins)
    n = shape[0]
    p = shape[1] if len(shape) == 2 else 1
    ctx, lib = context(device), _lib.load()
    ent = [None] * 3
    eptr = [None] * 3
    if entries:
        if dev:
            import torch
            ent = [torch.empty(shape, dtype=torch.float64, device=mean.device) for _ in range(3)]
            eptr = [a.data_ptr() for a in ent]
        else:
            ent = [np.empty(shape) for _ in range(3)]
            eptr = [a.ctypes.data for a in ent]
    lm, ls, ly = (_plane2(x, len(shape)) for x in (lm, ls, ly))
    crps, ld, mse, cov = np.empty(p), np.empty(p), np.empty(p), np.empty((la.size, p))
    hist = np.zeros((max(nb, 0), p), dtype=np.int64)
    cnt = [np.zeros(p, dtype=np.int64) for _ in range(3)]
    mem = _lib.GPAR_MEM_DEVICE if dev else _lib.GPAR_MEM_HOST
    with _after_torch(ctx, dev):
        ctx.check(lib.gpar_score_gaussian(
            ctx.h, n, p, mp_, lm[0], lm[1], sp, ls[0], ls[1], yp, ly[0], ly[1], int(la.size),
            _ptr(la), nb, mem, eptr[0], p, 1, eptr[1], p, 1, eptr[2], p, 1, _ptr(crps), _ptr(ld),
            _ptr(mse), _ptr(cov), _ptr(hist), _ptr(cnt[0]), _ptr(cnt[1]), _ptr(cnt[2])))
    return GaussianScores(crps, ld, mse, cov, hist, cnt[0], cnt[1], cnt[2],
                          tuple(float(x) for x in la), ent[0], ent[1], ent[2])


class Posterior:
    """gpar_fit_posterior's result: the fitted theta of every output and its q(u), kept on the
    device, so that predictions whose inference inputs arrive later (the chained sweep of
    GPAR_scaled_examples.jl:172 / eeg.jl:249,274) run only the V*-dependent half of
    get_gpar_scaled_predictions (gpar_posterior_predict).  Holds the problems' buffers (`keep`)
    alive: device problems' inputs are borrowed by the posterior."""

    def __init__(self, handle, fit, problems, keep, device):
        self.h, self.fit, self.device = handle, fit, device
        self._problems, self._keep = list(problems), keep
        self._prepared = {}   # output -> the t_star tensor a pending prepare reads

    @property
    def theta(self):
        return self.fit.theta

    def predict(self, i, t_star, V_star, mode="analytic", samples=100, seed=0):
        """Output i's (mean, std) at (t_star, V_star): device tensors (V_star N* x D, rows =
        points) for device problems, numpy (D x N* ColVecs) for host ones."""
        if not 0 <= int(i) < len(self._problems):
            raise _arg_error(f"output index {i} out of range (0..{len(self._problems) - 1})")
        p = self._problems[i]
        keep = _Keep()
        ctx, lib = context(self.device), _lib.load()
        md = _mode_id(mode)
        if p.mem == _lib.GPAR_MEM_DEVICE:
            import torch
            vsp, ldvs, ns, ds = _dev_points(V_star, keep)
            tsp = _dev_vec(t_star, keep)
            if ns != t_star.numel() or ds != p.d:
                raise _arg_error("inference inputs must be N* x D with N* = len(t_star)")
            mean = torch.empty(ns, dtype=torch.float64, device=t_star.device)
            std = torch.empty(ns, dtype=torch.float64, device=t_star.device)
            with _after_torch(ctx):
                ctx.check(lib.gpar_posterior_predict(ctx.h, self.h, int(i), ns, tsp, vsp, ldvs, md,
                                                     int(samples), int(seed), mean.data_ptr(),
                                                     std.data_ptr()))
            # the prepared slot is consumed (stream-ordered before any later use of the memory)
            self._prepared.pop(int(i), None)
            return mean, std
        vsp, ldvs, ns, ds = _host_points(V_star, keep)
        if ds != p.d or ns != len(np.asarray(t_star)):
            raise _arg_error("inference inputs must be D x N* with N* = len(t_star)")
        mean, std = np.zeros(ns), np.zeros(ns)
        ctx.check(lib.gpar_posterior_predict(ctx.h, self.h, int(i), ns, _host_vec(t_star, keep), vsp,
                                             ldvs, md, int(samples), int(seed), _ptr(mean), _ptr(std)))
        return mean, std

    def predict_mean(self, i, t_star, V_star):
        """Output i's analytic mean alone at (t_star, V_star) (gpar_posterior_predict_mean): the
        quantity a chained sweep passes on, without the variance's work.  Tensors as predict's."""
        if not 0 <= int(i) < len(self._problems):
            raise _arg_error(f"output index {i} out of range (0..{len(self._problems) - 1})")
        p = self._problems[i]
        keep = _Keep()
        ctx, lib = context(self.device), _lib.load()
        if p.mem == _lib.GPAR_MEM_DEVICE:
            import torch
            vsp, ldvs, ns, ds = _dev_points(V_star, keep)
            tsp = _dev_vec(t_star, keep)
            if ns != t_star.numel() or ds != p.d:
                raise _arg_error("inference inputs must be N* x D with N* = len(t_star)")
            mean = torch.empty(ns, dtype=torch.float64, device=t_star.device)
            with _after_torch(ctx):
                ctx.check(lib.gpar_posterior_predict_mean(ctx.h, self.h, int(i), ns, tsp, vsp, ldvs,
                                                          mean.data_ptr()))
            # the prepared slot is consumed (stream-ordered before any later use of the memory)
            self._prepared.pop(int(i), None)
            return mean
        vsp, ldvs, ns, ds = _host_points(V_star, keep)
        if ds != p.d or ns != len(np.asarray(t_star)):
            raise _arg_error("inference inputs must be D x N* with N* = len(t_star)")
        mean = np.zeros(ns)
        ctx.check(lib.gpar_posterior_predict_mean(ctx.h, self.h, int(i), ns,
                                                  _host_vec(t_star, keep), vsp, ldvs, _ptr(mean)))
        return mean

    def predict_samples(self, i, t_star, shared_inputs, sample_inputs, samples=None, seed=0,
                        out=None):
        """Output i's joint samples at per-sample inference inputs (gpar_posterior_predict_samples;
        arguments, layouts and the returned (F, mean, std) as predict_samples_scaled's).  Uses and
        consumes a matching prepare(i, t_star)."""
        if not 0 <= int(i) < len(self._problems):
            raise _arg_error(f"output index {i} out of range (0..{len(self._problems) - 1})")
        p = self._problems[i]
        ctx, lib = context(self.device), _lib.load()
        call = lambda *a: lib.gpar_posterior_predict_samples(ctx.h, self.h, int(i), *a)
        dev = p.mem == _lib.GPAR_MEM_DEVICE
        try:
            return _samples_call(call, dev, p.d, t_star, shared_inputs, sample_inputs, samples, seed,
                                 out, self.device)
        finally:
            if dev:   # the prepared slot is consumed (stream-ordered before any later use)
                self._prepared.pop(int(i), None)

    def sample_chain(self, t_star, given_inputs, samples, seed=0):
        """Joint samples of all outputs of a GPAR-ordered posterior -- output i's inputs are the
        d_given given columns followed by outputs 0..i-1, D_i = d_given + i -- at t_star: the chain
        p(y_0 | x) p(y_1 | x, y_0) ... sampled jointly, sample s of the earlier outputs feeding
        sample s of the later ones.  given_inputs: d_given x N* (host, ColVecs) / N* x d_given
        (device).  Allocates the S x N* x P chain tensor and sweeps the outputs in order: output i
        reads columns [:i] of every sample's slab in place, draws with seed + i (fit_predict_batch's
        convention) and writes column i.  Returns (samples S x N* x P, means, stds), means / stds
        lists of the per-output sample mean and Bessel std.  One rank only.
        sample_chain_quantiles adds the chain's credible bands."""
        P = len(self._problems)
        S = int(samples)
        dev = self._problems[0].mem == _lib.GPAR_MEM_DEVICE
        if dev:
            import torch
            ns = t_star.numel()
            given = given_inputs.reshape(ns, -1) if given_inputs.dim() == 1 else given_inputs
            dg = given.shape[1]
            chain = torch.empty((max(S, 0), ns, P), dtype=torch.float64, device=t_star.device)
        else:
            ns = len(np.asarray(t_star))
            given = to_colvecs(given_inputs)
            dg = given.shape[0]
            chain = np.zeros((max(S, 0), ns, P))
        for i, p in enumerate(self._problems):
            if p.d != dg + i:
                raise _arg_error(f"sample_chain: output {i} must have D = d_given + {i} = {dg + i} "
                                 f"inputs, has {p.d}")
        means, stds = [], []
        for i in range(P):
            _, m, s = self.predict_samples(i, t_star, given, chain[:, :, :i] if i else None,
                                           samples=S, seed=int(seed) + i, out=chain[:, :, i])
            means.append(m)
            stds.append(s)
        return chain, means, stds

    def sample_chain_quantiles(self, t_star, given_inputs, samples, quantiles, seed=0):
        """sample_chain with the chain's credible bands: returns (samples, means, stds, bands),
        the first three exactly sample_chain's for the same arguments, bands the len(quantiles) x
        N* x P quantiles of the chain over its samples at the levels `quantiles` (a sequence in
        [0, 1]) -- one sample_quantiles call over the whole chain tensor after the sweep, which
        reads it in place."""
        chain, means, stds = self.sample_chain(t_star, given_inputs, samples, seed=seed)
        return chain, means, stds, sample_quantiles(chain, quantiles, device=self.device)

    def sample_chain_scores(self, t_star, given_inputs, samples, y_star, levels=(0.5, 0.9, 0.95),
                            bins=10, seed=0):
        """sample_chain scored against held-out targets: returns (samples, means, stds, scores),
        the first three exactly sample_chain's for the same arguments, scores the SampleScores of
        the whole chain against y_star (N* x P, of the chain's memory kind, NaN where an output
        was not observed) -- one score_samples call after the sweep, which reads the chain in
        place."""
        chain, means, stds = self.sample_chain(t_star, given_inputs, samples, seed=seed)
        return chain, means, stds, score_samples(chain, y_star, levels=levels, bins=bins,
                                                 device=self.device)

    def prepare(self, i, t_star):
        """Queue output i's inference-input-independent prediction work for device test times
        t_star (gpar_posterior_prepare) on the context's side stream; the next predict(i, t_star,
        ...) with the same tensor uses it.  Device problems only.  The queued kernels read t_star
        asynchronously, so it must be contiguous (no temporary copy) and must not be freed or
        written until that predict has run: the Posterior holds a reference to it until then."""
        self._prepare(i, t_star, "gpar_posterior_prepare")

    def prepare_mean(self, i, t_star):
        """prepare, and also output i's training-side share of predict_mean if the posterior does
        not hold it yet (gpar_posterior_prepare_mean).  The next predict_mean(i, t_star, ...) or
        predict(i, t_star, ...) with the same tensor uses the slot; t_star as for prepare."""
        self._prepare(i, t_star, "gpar_posterior_prepare_mean")

    def _prepare(self, i, t_star, entry):
        if not 0 <= int(i) < len(self._problems):
            raise _arg_error(f"output index {i} out of range (0..{len(self._problems) - 1})")
        if self._problems[i].mem != _lib.GPAR_MEM_DEVICE:
            raise _arg_error("prepare: device-memory posteriors only")
        if not t_star.is_contiguous():
            raise _arg_error("prepare: t_star must be a contiguous device tensor (the prepared "
                             "kernels read it after this call returns)")
        ctx, lib = context(self.device), _lib.load()
        with _after_torch(ctx):
            ctx.check(getattr(lib, entry)(ctx.h, self.h, int(i), t_star.numel(), t_star.data_ptr()))
        # alive until the matching predict (two slots per context: at most two pending)
        self._prepared[int(i)] = t_star
        while len(self._prepared) > 2:
            self._prepared.pop(next(iter(self._prepared)))

    def close(self):
        if getattr(self, "h", None):
            _lib.load().gpar_posterior_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fit_posterior(problems, log_theta0, max_evals=0, max_iterations=1000, g_tol=1e-8,
                  time_limit=0.0, device=0, keep=None):
    """The fit and q(u) of get_gpar_scaled_predictions for a batch of outputs, kept on the device
    for later predictions (gpar_fit_posterior) -> Posterior.

    Device problems' buffers are borrowed by the posterior until it is closed, so their `keep`
    (the second value make_problem returns: the contiguous copies and columns the problems point
    at) is required and held by the Posterior.  Host problems are copied to the device."""
    ctx, lib = context(device), _lib.load()
    P = len(problems)
    if keep is None and any(p.mem == _lib.GPAR_MEM_DEVICE for p in problems):
        raise _arg_error("fit_posterior: device problems need their keep (make_problem's second "
                         "value): the posterior reads those buffers until it is closed")
    arr = (GparProblem * P)(*problems)
    x0 = np.ascontiguousarray(np.asarray(log_theta0, dtype=np.float64).reshape(P, 5))
    opts = GparFitOptions(int(max_evals), int(max_iterations), float(g_tol), float(time_limit))
    theta, nlml, evals = np.zeros((P, 5)), np.zeros(P), np.zeros(P, dtype=np.int32)
    h = C.c_void_p()
    with _after_torch(ctx, problems[0].mem == _lib.GPAR_MEM_DEVICE):
        ctx.check(lib.gpar_fit_posterior(ctx.h, arr, P, _ptr(x0), C.byref(opts), _ptr(theta),
                                         _ptr(nlml), _ptr(evals), C.byref(h)))
    return Posterior(h, FitResult(theta, nlml, evals), problems, keep, device)


def mc_normals(samples, m, seed, device=0):
    """The standard-normal draws MC-mode prediction uses for (samples, m, seed), samples x m
    (gpar_mc_normals): draw s maps to the pseudo-point sample m_e + chol(inv(D)).L xi_s
    (gpar_scaled_inference.jl:103,185).  fit_predict_batch draws output i with seed + i."""
    ctx = context(device)
    xi = np.zeros((int(samples), int(m)))
    ctx.check(_lib.load().gpar_mc_normals(ctx.h, int(samples), int(m), int(seed), _ptr(xi)))
    return xi


def path_normals(samples, n, d, seed, device=0):
    """The backward-sampling draws of posterior_rand / mode="path" for (samples, n, d, seed):
    samples x n x d (gpar_path_normals)."""
    ctx = context(device)
    xi = np.zeros((int(samples), int(n), int(d)))
    ctx.check(_lib.load().gpar_path_normals(ctx.h, int(samples), int(n), int(d), int(seed), _ptr(xi)))
    return xi


def posterior_rand(t, y, theta, kernel="matern52", samples=1, seed=0, noise=None, device=0):
    """TemporalGPs posterior_rand(rng, create_lgssm(t, l, pv, sigma, k; noise_vector), y, samples)
    (called at src/gp/tmp.jl:161-167): joint draws of the latent f over t from its posterior given
    y, by the Durbin-Koopman simulation smoother (gpar_lgssm_posterior_rand).  theta = (l,
    process_var, noise_sigma); noise: per-step observation variance (None: sigma^2).  Host arrays
    -> samples x n numpy array; torch CUDA tensors -> samples x n device tensor."""
    ctx, lib = context(device), _lib.load()
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(3))
    keep = _Keep()
    if _is_torch(t):
        import torch
        n = t.numel()
        # the C side cannot see device buffer lengths (as make_problem checks for the GPAR inputs)
        if y.numel() != n or (noise is not None and noise.numel() != n):
            raise _arg_error("t, y (and noise) must have the same length")
        out = torch.empty((int(samples), n), dtype=torch.float64, device=t.device)
        tp, yp = _dev_vec(t, keep), _dev_vec(y, keep)
        npp = _dev_vec(noise, keep) if noise is not None else None
        with _after_torch(ctx):
            ctx.check(lib.gpar_lgssm_posterior_rand(ctx.h, n, tp, yp, npp, _kernel_id(kernel),
                                                    _ptr(th), int(samples), int(seed),
                                                    _lib.GPAR_MEM_DEVICE, out.data_ptr()))
        return out
    n = len(np.asarray(t))
    if len(np.asarray(y)) != n or (noise is not None and len(np.asarray(noise)) != n):
        raise _arg_error("t, y (and noise) must have the same length")
    out = np.zeros((int(samples), n))
    ctx.check(lib.gpar_lgssm_posterior_rand(ctx.h, n, _host_vec(t, keep), _host_vec(y, keep),
                                            _host_vec(noise, keep) if noise is not None else None,
                                            _kernel_id(kernel), _ptr(th), int(samples), int(seed),
                                            _lib.GPAR_MEM_HOST, _ptr(out)))
    return out


def get_optim_scaled_gpar_params(input_locations, pseudo_input_locations, time_loc, outputs,
                                 out_kernel="matern52", time_kernel="matern52",
                                 i_log_time_l=None, i_log_time_var=None, i_log_out_l=None,
                                 i_log_out_var=None, i_log_noise_sigma=None,
                                 optimization_time_limit=DEFAULT_TIME_LIMIT, max_evals=0,
                                 g_tol=1e-8, rng=None, device=0):
    """dtc.jl:11-77: returns the optimised (time_l, time_var, out_l, out_var, noise_sigma)."""
    p, keep = make_problem(input_locations, pseudo_input_locations, time_loc, outputs,
                           out_kernel, time_kernel)
    x0 = parse_initial_params([i_log_time_l, i_log_time_var, i_log_out_l, i_log_out_var,
                               i_log_noise_sigma], rng)
    r = fit_batch([p], x0[None, :], max_evals=max_evals, g_tol=g_tol,
                  time_limit=optimization_time_limit or 0.0, device=device)
    return tuple(float(v) for v in r.theta[0])


# ----------------------------------------------------------------------------- q(u)
def compute_q_u(input_locations, pseudo_input_locations, time_loc, outputs, theta,
                out_kernel="matern52", time_kernel="matern52", device=0, qu_kuu_noise=False):
    """gpar_scaled_inference.jl:141-196 -> (m_e, cov_e = inv(D), U_u upper).  qu_kuu_noise:
    Cuu + sigma^2 I instead of the reference's noise-free Cuu (:157), as gpar_problem documents."""
    ctx = context(device)
    lib = _lib.load()
    p, keep = make_problem(input_locations, pseudo_input_locations, time_loc, outputs,
                           out_kernel, time_kernel, qu_kuu_noise=qu_kuu_noise)
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(5))
    m = p.m
    me = np.zeros(m)
    cov = np.zeros((m, m))
    U = np.zeros((m, m))  # column-major -> read as transposed
    with _after_torch(ctx, p.mem == _lib.GPAR_MEM_DEVICE):
        ctx.check(lib.gpar_q_u(ctx.h, C.byref(p), _ptr(th), _ptr(me), _ptr(cov), _ptr(U)))
    return me, cov, U.T.copy()


# ----------------------------------------------------------------------------- temporal-only
@dataclass
class LGSSMSpec:
    """create_lgssm(t, l, process_var, noise_sigma, k) (temporal_gp_inference.jl:15-39)."""
    t: np.ndarray
    l: float
    process_var: float
    noise_sigma: float
    kernel: str = "matern52"


def create_lgssm(latent_locations, l, process_var, noise_sigma, kernel_structure="matern52"):
    return LGSSMSpec(np.asarray(latent_locations, dtype=np.float64), float(l), float(process_var),
                     float(noise_sigma), kernel_structure)


def logpdf(lgssm: LGSSMSpec, y, device=0):
    """logpdf(lgssm, y) (temporal_gp_inference.jl:78)."""
    return float(lgssm_logpdf_batch(lgssm.t, np.asarray(y, dtype=np.float64)[None, :],
                                    [[lgssm.l, lgssm.process_var, lgssm.noise_sigma]],
                                    lgssm.kernel, device)[0])


def lgssm_logpdf_batch(t, Y, theta, kernel="matern52", device=0):
    """Chains sharing t: Y is nchains x n; theta nchains x 3 natural (l, pv, sigma)."""
    ctx = context(device)
    lib = _lib.load()
    keep = _Keep()
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64))
    nch, n = Y.shape
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(nch, 3))
    tp = _host_vec(t, keep)
    out = np.zeros(nch)
    ctx.check(lib.gpar_lgssm_logpdf(ctx.h, nch, n, tp, _ptr(Y), n, _kernel_id(kernel), _ptr(th),
                                    _lib.GPAR_MEM_HOST, _ptr(out)))
    return out


# ----------------------------------------------------------------------------- prediction
def predict_scaled(input_locations, pseudo_input_locations, time_loc, outputs, theta,
                   inference_time_loc, inference_input_locations, out_kernel="matern52",
                   time_kernel="matern52", mode="analytic", samples=100, seed=0, device=0,
                   qu_kuu_noise=False):
    """Prediction half of get_gpar_scaled_predictions (gpar_scaled_inference.jl:63-135) at a
    given theta.  Returns (mean, std) at the inference locations, in their input order.
    mode="mc" reproduces the reference's 100-sample Monte Carlo estimator; "analytic" is its
    S -> infinity limit."""
    p, keep = make_problem(input_locations, pseudo_input_locations, time_loc, outputs,
                           out_kernel, time_kernel, qu_kuu_noise=qu_kuu_noise)
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(5))
    md = _mode_id(mode)
    if p.mem == _lib.GPAR_MEM_DEVICE:
        import torch
        vsp, ldvs, ns, ds = _dev_points(inference_input_locations, keep)
        tsp = _dev_vec(inference_time_loc, keep)
        if ns != inference_time_loc.numel() or ds != p.d:
            raise _arg_error("inference inputs must be N* x D with N* = len(inference_time_loc)")
        ctx, lib = context(device), _lib.load()
        mean = torch.empty(ns, dtype=torch.float64, device=inference_time_loc.device)
        std = torch.empty(ns, dtype=torch.float64, device=inference_time_loc.device)
        with _after_torch(ctx):
            ctx.check(lib.gpar_predict(ctx.h, C.byref(p), _ptr(th), ns, tsp, vsp, ldvs, md,
                                       int(samples), int(seed), mean.data_ptr(), std.data_ptr()))
        return mean, std
    vsp, ldvs, ns, ds = _host_points(inference_input_locations, keep)
    tsp = _host_vec(inference_time_loc, keep)
    if ds != p.d or ns != len(np.asarray(inference_time_loc)):
        raise _arg_error("inference inputs must have the training dimension and one point per "
                         "inference time")
    ctx, lib = context(device), _lib.load()
    mean = np.zeros(ns)
    std = np.zeros(ns)
    ctx.check(lib.gpar_predict(ctx.h, C.byref(p), _ptr(th), ns, tsp, vsp, ldvs, md, int(samples),
                               int(seed), _ptr(mean), _ptr(std)))
    return mean, std


def predict_mean_scaled(input_locations, pseudo_input_locations, time_loc, outputs, theta,
                        inference_time_loc, inference_input_locations, out_kernel="matern52",
                        time_kernel="matern52", device=0, qu_kuu_noise=False):
    """The analytic mean of predict_scaled alone (gpar_predict_mean): what a chain of outputs
    passes on (GPAR_scaled_examples.jl:172), at O((N + N*) M D) instead of O(N* M^2).  Returns the
    mean at the inference locations, in their input order.  Not the "mc" / "path" sample means."""
    p, keep = make_problem(input_locations, pseudo_input_locations, time_loc, outputs,
                           out_kernel, time_kernel, qu_kuu_noise=qu_kuu_noise)
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(5))
    if p.mem == _lib.GPAR_MEM_DEVICE:
        import torch
        vsp, ldvs, ns, ds = _dev_points(inference_input_locations, keep)
        tsp = _dev_vec(inference_time_loc, keep)
        if ns != inference_time_loc.numel() or ds != p.d:
            raise _arg_error("inference inputs must be N* x D with N* = len(inference_time_loc)")
        ctx, lib = context(device), _lib.load()
        mean = torch.empty(ns, dtype=torch.float64, device=inference_time_loc.device)
        with _after_torch(ctx):
            ctx.check(lib.gpar_predict_mean(ctx.h, C.byref(p), _ptr(th), ns, tsp, vsp, ldvs,
                                            mean.data_ptr()))
        return mean
    vsp, ldvs, ns, ds = _host_points(inference_input_locations, keep)
    tsp = _host_vec(inference_time_loc, keep)
    if ds != p.d or ns != len(np.asarray(inference_time_loc)):
        raise _arg_error("inference inputs must have the training dimension and one point per "
                         "inference time")
    ctx, lib = context(device), _lib.load()
    mean = np.zeros(ns)
    ctx.check(lib.gpar_predict_mean(ctx.h, C.byref(p), _ptr(th), ns, tsp, vsp, ldvs, _ptr(mean)))
    return mean


def get_gpar_scaled_predictions(input_locations, pseudo_input_locations, time_loc, outputs,
                                inference_time_loc, inference_input_locations,
                                out_kernel_structure="matern52", time_kernel_structure="matern52",
                                i_log_time_l=None, i_log_time_var=None, i_log_out_l=None,
                                i_log_out_var=None, i_log_noise_sigma=None,
                                optimization_time_limit=DEFAULT_TIME_LIMIT, max_evals=0,
                                mode="mc", samples=100, seed=0, rng=None, device=0):
    """gpar_scaled_inference.jl:20-136: fit theta (Matern52 hard-coded for the fit, :48-49),
    then predict; returns (mean, std) like the reference."""
    theta = get_optim_scaled_gpar_params(
        input_locations, pseudo_input_locations, time_loc, outputs, "matern52", "matern52",
        i_log_time_l, i_log_time_var, i_log_out_l, i_log_out_var, i_log_noise_sigma,
        optimization_time_limit, max_evals, rng=rng, device=device)
    return predict_scaled(input_locations, pseudo_input_locations, time_loc, outputs, theta,
                          inference_time_loc, inference_input_locations, out_kernel_structure,
                          time_kernel_structure, mode, samples, seed, device)


def lgssm_smooth_batch(t, Y, theta, kernel="matern52", noise=None, device=0):
    """smooth(create_lgssm(...; noise_vector), y) marginals of f for chains sharing t
    (temporal_gp_inference.jl:109): returns (mean, var), nchains x n."""
    ctx = context(device)
    lib = _lib.load()
    keep = _Keep()
    Y = np.ascontiguousarray(np.atleast_2d(np.asarray(Y, dtype=np.float64)))
    nch, n = Y.shape
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(nch, 3))
    tp = _host_vec(t, keep)
    npp = _host_vec(noise, keep) if noise is not None else None
    mean = np.zeros((nch, n))
    var = np.zeros((nch, n))
    ctx.check(lib.gpar_lgssm_smooth(ctx.h, nch, n, tp, _ptr(Y), n, npp, _kernel_id(kernel),
                                    _ptr(th), _lib.GPAR_MEM_HOST, _ptr(mean), _ptr(var)))
    return mean, var


def get_sde_predictions(data_locations, data_outputs, output_locations,
                        kernel_structure="matern52", i_log_time_l=None, i_log_time_var=None,
                        i_log_noise_sigma=None, max_evals=0, g_tol=1e-8, time_limit=0.0,
                        rng=None, device=0):
    """temporal_gp_inference.jl:45-114 for one or several chains sharing the time grid.

    data_outputs: n (one chain) or nchains x n.  Returns (theta, mean, var) with the
    marginals of f at output_locations (the reference returns their Gaussians; its
    `.m[1]` / `.P[1]` are mean / variance)."""
    ctx = context(device)
    lib = _lib.load()
    keep = _Keep()
    Y = np.ascontiguousarray(np.atleast_2d(np.asarray(data_outputs, dtype=np.float64)))
    nch, n = Y.shape
    x0 = np.vstack([parse_initial_params([i_log_time_l, i_log_time_var, i_log_noise_sigma], rng)
                    for _ in range(nch)])
    x0 = np.ascontiguousarray(x0)
    ts = np.asarray(output_locations, dtype=np.float64)
    tp = _host_vec(data_locations, keep)
    tsp = _host_vec(ts, keep)
    opts = GparFitOptions(int(max_evals), 1000, float(g_tol), float(time_limit))
    theta = np.zeros((nch, 3))
    mean = np.zeros((nch, len(ts)))
    var = np.zeros((nch, len(ts)))
    ctx.check(lib.gpar_sde_predictions(ctx.h, nch, n, tp, _ptr(Y), n, len(ts), tsp,
                                       _kernel_id(kernel_structure), _ptr(x0), C.byref(opts),
                                       _lib.GPAR_MEM_HOST, _ptr(theta), _ptr(mean), _ptr(var)))
    if nch == 1:
        return tuple(theta[0]), mean[0], var[0]
    return theta, mean, var


def get_sde_predictions_device(t, Y, t_star, kernel_structure="matern52", log_theta0=(0.0, 0.0, -2.0),
                               max_evals=0, g_tol=-1.0, time_limit=0.0, device=0):
    """get_sde_predictions with HBM-resident torch inputs: t (n), Y (n) or (nchains x n,
    contiguous rows), t_star (n_star, ascending).  Returns (theta, mean, var) on the device."""
    import torch
    ctx = context(device)
    lib = _lib.load()
    keep = _Keep()
    Y2 = Y.reshape(1, -1) if Y.dim() == 1 else Y
    Y2 = Y2.contiguous()
    nch, n = Y2.shape
    x0 = np.ascontiguousarray(np.tile(np.asarray(log_theta0, dtype=np.float64), (nch, 1)))
    opts = GparFitOptions(int(max_evals), 1000, float(g_tol), float(time_limit))
    theta = np.zeros((nch, 3))
    ns = t_star.shape[0]
    mean = torch.empty((nch, ns), dtype=torch.float64, device=t.device)
    var = torch.empty((nch, ns), dtype=torch.float64, device=t.device)
    if t.numel() != n:
        raise _arg_error("t and Y must have the same length")
    ts_ = _dev_vec(t_star, keep)
    tt_ = _dev_vec(t, keep)
    with _after_torch(ctx):
        ctx.check(lib.gpar_sde_predictions(ctx.h, nch, n, tt_, Y2.data_ptr(), n, ns,
                                           ts_, _kernel_id(kernel_structure),
                                           _ptr(x0), C.byref(opts), _lib.GPAR_MEM_DEVICE,
                                           _ptr(theta), mean.data_ptr(), var.data_ptr()))
    if nch == 1:
        return tuple(theta[0]), mean[0], var[0]
    return theta, mean, var


# ----------------------------------------------------------------------------- exact GP / GPAR
def _theta5(theta, dx):
    th = np.asarray(theta, dtype=np.float64).ravel()
    if dx == 1 and th.shape[0] == 3:        # unpack_gp order (l, process_var, noise_sigma)
        th = np.array([th[0], th[1], 1.0, 1.0, th[2]])
    return np.ascontiguousarray(th.reshape(5))


def exact_logpdf(X, y, theta, time_kernel="eq", out_kernel="eq", device=0):
    """logpdf(f(x, sigma^2), y) of the exact GP (dx == 1, optimized.jl:28-36, theta =
    (l, process_var, noise_sigma)) or GPAR (optimized.jl:132-154, theta = unpack_gpar order).
    X: 1-D times or ColVecs dx x n with row 0 = time."""
    ctx = context(device)
    keep = _Keep()
    xp, ldx, n, dx = _host_points(X, keep)
    th = _theta5(theta, dx)
    out = np.zeros(1)
    ctx.check(_lib.load().gpar_exact_logpdf(ctx.h, n, dx, xp, ldx, _host_vec(y, keep),
                                            _kernel_id(time_kernel), _kernel_id(out_kernel),
                                            _ptr(th), _lib.GPAR_MEM_HOST, _ptr(out)))
    return float(out[0])


def exact_posterior(X, y, X_star, theta, time_kernel="eq", out_kernel="eq", device=0):
    """Marginals (mean, var) of f at X_star under the exact posterior
    gp | (gp(x, sigma^2) <- y)  (optimized.jl:94,236)."""
    ctx = context(device)
    keep = _Keep()
    xp, ldx, n, dx = _host_points(X, keep)
    sp, ldxs, ns, dxs = _host_points(X_star, keep)
    if dxs != dx:
        raise _lib.DomainError(_lib.GPAR_ERR_ARG, "X_star must have the dimension of X")
    th = _theta5(theta, dx)
    mean = np.zeros(ns)
    var = np.zeros(ns)
    ctx.check(_lib.load().gpar_exact_posterior(ctx.h, n, dx, xp, ldx, _host_vec(y, keep), ns, sp,
                                               ldxs, _kernel_id(time_kernel), _kernel_id(out_kernel),
                                               _ptr(th), _lib.GPAR_MEM_HOST, _ptr(mean), _ptr(var)))
    return mean, var


@dataclass
class ExactGP:
    """Result of create_optim_gp[ar]: the fitted kernel (the reference returns the Stheno GP
    and opt_params)."""
    X: np.ndarray
    y: np.ndarray
    theta: tuple
    time_kernel: str
    out_kernel: str
    device: int = 0

    def logpdf(self):
        return exact_logpdf(self.X, self.y, self.theta, self.time_kernel, self.out_kernel, self.device)

    def marginals(self, X_star):
        """Posterior marginals (mean, var) at X_star: the create_optim_gp[ar]_post posterior."""
        return exact_posterior(self.X, self.y, X_star, self.theta, self.time_kernel,
                               self.out_kernel, self.device)


def _nm_fit(nlml, x0, max_evals):
    nm = _lib.NelderMead(x0, max_evals=max_evals)
    while (x := nm.ask()) is not None:
        try:
            f = nlml(x)
        except _lib.PosDefException:
            f = np.inf
        nm.tell(f)
    return nm.result()[0]


def create_optim_gp(input_locations, outputs, kernel_structure="eq", i_log_l=None,
                    i_log_process_var=None, i_log_noise_sigma=None, max_evals=0, rng=None, device=0):
    """optimized.jl:19-59: NelderMead on -logpdf over (l, process_var, noise_sigma);
    returns (ExactGP, opt_params)."""
    x = np.asarray(input_locations, dtype=np.float64).ravel()
    y = np.asarray(outputs, dtype=np.float64)
    x0 = parse_initial_params([i_log_l, i_log_process_var, i_log_noise_sigma], rng)
    xm = _nm_fit(lambda p: -exact_logpdf(x, y, unpack_gp(p), kernel_structure, device=device),
                 x0, max_evals)
    th = unpack_gp(xm)
    return ExactGP(x, y, th, kernel_structure, kernel_structure, device), th


def create_optim_gpar(input_locations, outputs, time_kernel="eq", out_kernel="eq",
                      i_log_time_l=None, i_log_time_var=None, i_log_out_l=None,
                      i_log_out_var=None, i_log_noise_sigma=None, multi_input=True, max_evals=0,
                      rng=None, device=0):
    """optimized.jl:106-183 (multi_input=False falls back to create_optim_gp, :118-127)."""
    if not multi_input:
        return create_optim_gp(input_locations, outputs, time_kernel, i_log_time_l, i_log_time_var,
                               i_log_noise_sigma, max_evals, rng, device)
    X = to_colvecs(input_locations)
    y = np.asarray(outputs, dtype=np.float64)
    x0 = parse_initial_params([i_log_time_l, i_log_time_var, i_log_out_l, i_log_out_var,
                               i_log_noise_sigma], rng)
    xm = _nm_fit(lambda p: -exact_logpdf(X, y, unpack_gpar(p), time_kernel, out_kernel, device),
                 x0, max_evals)
    th = unpack_gpar(xm)
    return ExactGP(X, y, th, time_kernel, out_kernel, device), th


def create_optim_gp_post(input_locations, outputs, kernel_structure="eq", **kw):
    """optimized.jl:76-97: the fitted GP conditioned on the data (use .marginals(x_star))."""
    return create_optim_gp(input_locations, outputs, kernel_structure, **kw)[0]


def create_optim_gpar_post(input_locations, outputs, time_kernel="eq", out_kernel="eq", **kw):
    """optimized.jl:201-239."""
    return create_optim_gpar(input_locations, outputs, time_kernel, out_kernel, **kw)[0]
