"""Quantiles over the sample axis on the GPU (gpar_sample_quantiles, k_quantile.hip).

Reference: np.quantile(F, q, axis=0) (numpy's default method, "linear").  With x the ascending sort
of an entry's S samples, h = q (S - 1), lo = floor(h), g = h - lo, a = x[lo], b = x[min(lo + 1,
S - 1)]:
  * where g = 0 or a = b the result is the sorted sample a, bit for bit;
  * elsewhere |result - numpy| <= 6 * 2^-52 * max(|a|, |b|): either form of the interpolation makes
    three roundings of quantities bounded by 2 max(|a|, |b|), at most 2.5 * 2^-52 max per
    implementation, 5 between two, plus one of slack (derived, not measured);
  * an entry with a NaN sample gives NaN for every q.
The register path serves S <= 128 (its four instantiations, 16 / 32 / 64 / 128 registers, compile
without scratch), the LDS path 129..4096; the launch counters say which one ran, and
GPAR_QUANTILE_PATH forces either where both can serve.  Strided views, host memory and repeated
calls give the packed device call's bits."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

REG_MAX = 128   # the register path's cut-over (kQuantRegMax, launch.hpp)
Q5 = (0.0, 0.025, 0.5, 0.975, 1.0)
Q_UNSORTED = (0.9, 0.1, 0.5, 0.1, 1.0, 0.0, 0.33, 0.9)
SIZES = (1, 2, 3, 15, 16, 17, 33, 64, 65, 100, 128, 129, 1000, 4096)
SHAPES = ((1, 1), (63, 1), (64, 1), (65, 1), (77, 3), (300, 5))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _counters():
    return G.debug_counter("quantile_reg"), G.debug_counter("quantile_lds")


@functools.lru_cache(maxsize=None)
def _samples(S, n, p, seed=0):
    F = np.random.default_rng(1000 * S + 10 * n + p + seed).standard_normal((S, n, p))
    F.setflags(write=False)
    return F


def _check(F, q, got):
    """got against the definition (exact cases) and numpy (interpolated cases), printed first"""
    S = F.shape[0]
    got = np.asarray(got)
    assert got.shape == (len(q),) + F.shape[1:]
    x = np.sort(F, axis=0)
    nan = np.isnan(F).any(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.quantile(F, q, axis=0)
        worst = 0.0
        for j, qj in enumerate(q):
            h = qj * (S - 1)
            lo = int(np.floor(h))
            g = h - lo
            a, b = x[lo], x[min(lo + 1, S - 1)]
            exact = ((g == 0.0) | (a == b)) & ~nan
            rest = ~exact & ~nan
            assert np.array_equal(_bits(got[j][exact]), _bits(a[exact])), (S, qj)
            tol = 6 * 2.0 ** -52 * np.maximum(np.abs(a), np.abs(b))
            err = np.abs(got[j] - ref[j])
            same = (got[j] == ref[j]) | (np.isnan(got[j]) & np.isnan(ref[j]))
            if rest.any() and np.isfinite(err[rest & ~same]).any():
                worst = max(worst, float(np.nanmax((err / tol)[rest & ~same])))
            assert np.all(same[rest] | (err[rest] <= tol[rest])), (S, qj, float(np.nanmax(err[rest])))
            assert np.all(np.isnan(got[j][nan])), (S, qj)
    print(f"S={S} shape={F.shape[1:]} worst |got - numpy| / tolerance = {worst:.3f}")


@pytest.mark.parametrize("np_", SHAPES, ids=lambda s: f"n{s[0]}p{s[1]}")
@pytest.mark.parametrize("S", SIZES)
def test_sizes_against_numpy_on_the_expected_path(S, np_):
    import torch
    n, p = np_
    F = _samples(S, n, p)
    Fd = torch.tensor(F, device="cuda")
    r0, l0 = _counters()
    got = G.sample_quantiles(Fd, Q5)
    r1, l1 = _counters()
    if S <= REG_MAX:
        assert r1 > r0 and l1 == l0, "the register path serves S <= 128"
    else:
        assert l1 > l0 and r1 == r0, "the LDS path serves S > 128"
    _check(F, Q5, got.cpu().numpy())
    got2 = G.sample_quantiles(Fd, Q_UNSORTED)
    _check(F, Q_UNSORTED, got2.cpu().numpy())
    # a level's result does not depend on the other levels of the call
    assert torch.equal(got2[2], got[2]) and torch.equal(got2[1], got2[3])


def test_integer_positions_return_the_sorted_samples():
    import torch
    F = _samples(101, 77, 3)
    q = tuple(k / 100 for k in range(101))
    got = G.sample_quantiles(torch.tensor(F, device="cuda"), q).cpu().numpy()
    _check(F, q, got)
    x = np.sort(F, axis=0)
    for k in range(101):
        h = q[k] * 100
        if h == np.floor(h):
            assert np.array_equal(_bits(got[k]), _bits(x[int(h)]))


@pytest.mark.parametrize("S", (1, 2, 16, 33, 100, 128))
def test_both_paths_agree_bit_for_bit(S, monkeypatch):
    import torch
    F = _samples(S, 77, 3)
    Fd = torch.tensor(F, device="cuda")
    out = {}
    for path in ("reg", "lds"):
        monkeypatch.setenv("GPAR_QUANTILE_PATH", path)
        r0, l0 = _counters()
        out[path] = G.sample_quantiles(Fd, Q_UNSORTED)
        r1, l1 = _counters()
        assert (r1 > r0, l1 > l0) == (path == "reg", path == "lds")
    assert torch.equal(out["reg"], out["lds"])
    _check(F, Q_UNSORTED, out["lds"].cpu().numpy())


def test_forcing_the_register_path_leaves_long_lists_to_lds(monkeypatch):
    import torch
    F = _samples(129, 65, 1)
    monkeypatch.setenv("GPAR_QUANTILE_PATH", "reg")
    r0, l0 = _counters()
    got = G.sample_quantiles(torch.tensor(F, device="cuda"), Q5)
    r1, l1 = _counters()
    assert r1 == r0 and l1 > l0
    _check(F, Q5, got.cpu().numpy())


def _special_values(S):
    """ties, all-equal lists, +-inf, NaNs in the first / a middle / the last sample, 1e-300..1e300"""
    rng = np.random.default_rng(7 + S)
    n, p = 40, 3
    F = rng.standard_normal((S, n, p))
    # ties; + 0.0 turns the -0.0 that rounding makes into +0.0 (the two compare equal, so "the
    # sorted list" does not say which of them sits where)
    F[:, 0] = np.round(F[:, 0] * 2) / 2 + 0.0
    F[:, 1] = 3.25                                           # all equal
    F[:, 2, 0] = rng.integers(0, 3, S)                       # few distinct values
    F[:, 3] = 10.0 ** rng.uniform(-300, 300, (S, p)) * rng.choice([-1.0, 1.0], (S, p))
    F[:, 4] = 10.0 ** rng.uniform(-300, -290, (S, p))
    if S >= 3:
        F[0, 5, 0] = np.inf
        F[S // 2, 5, 1] = -np.inf
        F[0, 5, 2], F[S - 1, 5, 2] = -np.inf, np.inf
        F[:, 6, 0] = np.inf                                  # all +inf
        F[: S // 2, 6, 1] = -np.inf                          # half -inf
    F[0, 8, 0] = np.nan                                      # first sample
    F[S // 2, 9, 1] = np.nan                                 # a middle sample
    F[S - 1, 10, 2] = np.nan                                 # the last sample
    F[:, 11, 1] = np.nan                                     # all NaN
    return F


@pytest.mark.parametrize("S", (1, 3, 16, 17, 100, 129, 1000))
def test_special_values(S):
    import torch
    F = _special_values(S)
    got = G.sample_quantiles(torch.tensor(F, device="cuda"), Q_UNSORTED).cpu().numpy()
    _check(F, Q_UNSORTED, got)
    nan = np.isnan(F).any(axis=0)
    assert nan.sum() == 4
    # the NaN entries' neighbours are untouched: only those entries are NaN, except where the
    # definition itself gives inf - inf
    clean = F.copy()
    clean[:, nan] = 0.0
    ref = G.sample_quantiles(torch.from_numpy(clean).cuda(), Q_UNSORTED).cpu().numpy()
    assert np.array_equal(_bits(got[:, ~nan]), _bits(ref[:, ~nan]))
    assert np.all(np.isnan(got[:, nan]))
    assert got[:, 1].min() == got[:, 1].max() == 3.25


@pytest.mark.parametrize("S", (16, 100, 200))
def test_layouts_and_memory_kinds_give_the_packed_bits(S):
    import torch
    n, P = 90, 5
    F = _samples(S, n, P, seed=3)
    chain = torch.tensor(F, device="cuda")
    packed = G.sample_quantiles(chain, Q5)
    assert torch.equal(packed, G.sample_quantiles(chain, Q5))          # two identical calls
    _check(F, Q5, packed.cpu().numpy())
    # a column of the wider tensor, read in place (ld_r = P)
    col = chain[:, :, 2]
    assert col.stride() == (n * P, P)
    got = G.sample_quantiles(col, Q5)
    assert tuple(got.shape) == (5, n) and torch.equal(got, packed[:, :, 2])
    assert torch.equal(got, G.sample_quantiles(col.contiguous(), Q5))
    # a row block, and a block of columns
    assert torch.equal(G.sample_quantiles(chain[:, 13:71], Q5), packed[:, 13:71])
    assert torch.equal(G.sample_quantiles(chain[:, :, 1:4], Q5), packed[:, :, 1:4])
    # every other sample: the packed copy's bits
    assert torch.equal(G.sample_quantiles(chain[::2], Q5),
                       G.sample_quantiles(chain[::2].contiguous(), Q5))
    # samples innermost (a transposed view)
    tr = chain.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert tr.stride() == (1, P * S, S)
    assert torch.equal(G.sample_quantiles(tr, Q5), packed)
    # out as a strided view
    big = torch.full((5, n, 2 * P + 1), -7.0, dtype=torch.float64, device="cuda")
    view = big[:, :, 1::2]
    assert G.sample_quantiles(chain, Q5, out=view) is view
    assert torch.equal(view, packed) and bool((big[:, :, 0::2] == -7.0).all())
    # host memory: the same bits, in place and into a strided out
    host = G.sample_quantiles(F, Q5)
    assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(packed.cpu().numpy()))
    hcol = G.sample_quantiles(F[:, :, 2], Q5)
    assert np.array_equal(_bits(hcol), _bits(host[:, :, 2]))
    hbig = np.full((5, 2 * n, P), -7.0)
    G.sample_quantiles(F, Q5, out=hbig[:, ::2])
    assert np.array_equal(_bits(hbig[:, ::2]), _bits(host)) and np.all(hbig[:, 1::2] == -7.0)


def test_device_call_takes_no_workspace_and_reports_its_bytes():
    import torch
    S, n, p = 100, 300, 5
    Fd = torch.tensor(_samples(S, n, p), device="cuda")
    ctx = G.context(0)
    G.sample_quantiles(Fd, Q5)
    before = ctx.workspace_bytes()
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        G.sample_quantiles(Fd, Q5)
        launches, ms = ctx.kernel_stats("quantile")
        assert launches == 1 and ms > 0.0
        assert ctx.kernel_work("quantile") == 8.0 * S * n * p
    finally:
        ctx.set_profiling(False)
    assert ctx.workspace_bytes() == before


def test_errors_launch_nothing():
    import torch
    F = _samples(16, 64, 1)
    Fd = torch.tensor(F, device="cuda")
    c0 = _counters()
    with pytest.raises(G.Unsupported):
        G.sample_quantiles(torch.zeros((4097, 3), dtype=torch.float64, device="cuda"), Q5)
    with pytest.raises(G.Unsupported):
        G.sample_quantiles(np.zeros((4097, 3)), Q5)
    for q in ((-0.1,), (1.1,), (float("nan"),), ()):
        with pytest.raises(G.DomainError):
            G.sample_quantiles(Fd, q)
        with pytest.raises(G.DomainError):
            G.sample_quantiles(F, q)
    # strides under which two entries share an address: F, then out
    flat = torch.arange(4096, dtype=torch.float64, device="cuda")
    for size, stride in (((16, 64, 2), (64, 1, 1)), ((16, 64, 2), (32, 2, 1)),
                         ((16, 64), (1, 1)), ((16, 64, 2), (128, 2, 2))):
        with pytest.raises(G.DomainError):
            G.sample_quantiles(torch.as_strided(flat, size, stride), Q5)
    with pytest.raises(G.DomainError):
        G.sample_quantiles(Fd, Q5, out=torch.as_strided(flat, (5, 64, 1), (32, 1, 1)))
    hflat = np.arange(4096.0)
    with pytest.raises(G.DomainError):
        G.sample_quantiles(np.lib.stride_tricks.as_strided(hflat, (16, 64, 2), (512, 8, 8)), Q5)
    assert _counters() == c0
    # an admissible interleaving is not an alias: rows of two columns, columns 64 apart
    ok = torch.as_strided(flat, (16, 64, 2), (128, 1, 64))
    assert torch.equal(G.sample_quantiles(ok, Q5), G.sample_quantiles(ok.contiguous(), Q5))


@functools.lru_cache(maxsize=None)
def _posterior():
    """three outputs in the GPAR ordering on the device (test_gpu_sample_chain.py's builder at
    n = 300, M = 32, N* = 50): output i reads the given column and outputs 0..i-1"""
    import torch
    from oracle import gpar_oracle as O
    t, Y = O.synthetic_gpar(300, 4, seed=21, noise=0.3)
    ts = np.sort(np.random.default_rng(4).uniform(t[0], t[-1], 50))
    Yd = torch.from_numpy(Y).cuda()
    td, tsd = torch.from_numpy(t).cuda(), torch.from_numpy(ts).cuda()
    given = torch.from_numpy(np.interp(ts, t, Y[:, 0])).cuda().reshape(-1, 1)
    probs, keep = [], G.api._Keep()
    for i in range(3):
        Z = torch.from_numpy(np.ascontiguousarray(
            O.pick_pseudo_inputs(Y[:, :1 + i].T, 32, 5 + i).T)).cuda()
        pr, k = G.make_problem(Yd[:, :1 + i], Z, td, Yd[:, 1 + i].contiguous())
        probs.append(pr)
        keep.append(k)
        keep.append(Z)
    x0 = np.tile([0.0, 0.0, 0.0, 0.0, -2.0], (3, 1))
    post = G.fit_posterior(probs, x0, max_evals=12, g_tol=-1.0, keep=keep)
    return post, tsd, given


def test_sample_chain_bands_end_to_end():
    import torch
    post, tsd, given = _posterior()
    S, q = 16, (0.1, 0.5, 0.9)
    plain = post.sample_chain(tsd, given, S, seed=40)
    assert len(plain) == 3
    chain, means, stds, bands = post.sample_chain_quantiles(tsd, given, S, q, seed=40)
    assert torch.equal(chain, plain[0])
    for a, b in zip(means + stds, plain[1] + plain[2]):
        assert torch.equal(a, b)
    assert tuple(bands.shape) == (3, 50, 3)
    _check(chain.cpu().numpy(), q, bands.cpu().numpy())
    assert bool((bands[0] <= bands[1]).all()) and bool((bands[1] <= bands[2]).all())
