"""Scores of predictions against held-out targets on the GPU (gpar_score_samples,
gpar_score_gaussian, k_score.hip), against numpy references written here.

Sample scorer, per entry with x the ascending sort of its S samples and d_k = x_k - y:
  * below = #{F_s < y}, equal = #{F_s == y}, the PIT bin min(B - 1, ((2 below + equal) B) // (2 S)),
    the histogram, scored / missing / bad and the inside counts are integers and must be exact;
  * crps = (1/S) sum |d_k| - (1/S^2) sum (2k - S + 1) d_k against the same formula in np.longdouble
    (and, for S <= 200, against the O(S^2) form mean|x - y| - mean|x - x'| / 2) within
    2 (S + 4) 2^-52 mean_k |d_k|: each of the two sums is within gamma_{S+2} of its sum of magnitudes
    for any summation order, |2k - S + 1| / S <= 1, and two implementations are compared (derived,
    not measured);
  * the aggregate crps against the mean of the per-entry values within (n + 2) 2^-52 mean (all
    terms non-negative);
  * the inside flag of level l equals (lo <= y) & (y <= hi) with lo, hi = sample_quantiles(F,
    ((1 - l) / 2, (1 + l) / 2)), exactly, targets equal to lo and to hi included.
The register path serves S <= 64 (the NP = 128 instantiation would spill beside the two sums), the
LDS path 65..4096; both give the same bits, as do strided views, host memory and repeated calls.

Gaussian scorer against math.erf / math.exp / math.log in fp64: the worst relative errors measured
on an MI355X were 6.1e-16 (crps), 7.8e-16 (log density, relative to its two terms' magnitudes) and 0
(squared error) at (n, p) = (300, 5); the test asserts 16 x the largest, far below the project's 1e-9."""
import ctypes as C
import functools
import math
from statistics import NormalDist

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

REG_MAX = 64    # the scorer's register cut-over (kScoreRegMax, launch.hpp)
CHUNK = 256     # points of one output per reduction chunk (kScoreChunk)
LEVELS = (0.5, 0.9, 0.95)
BINS = 10
SIZES = (1, 2, 3, 16, 17, 33, 64, 65, 100, 128, 129, 1000, 4096)
SHAPES = ((1, 1), (63, 1), (65, 1), (77, 3), (300, 5))
EPS = 2.0 ** -52
# worst relative error of the Gaussian scorer's per-entry values against the host evaluation,
# measured on an MI355X, and the asserted bound
GAUSS_MEASURED = 7.8e-16
GAUSS_RTOL = min(16 * GAUSS_MEASURED, 1e-9)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _counters():
    return G.debug_counter("score_reg"), G.debug_counter("score_lds")


def _band_levels(levels):
    q = []
    for l in levels:
        q += [(1 - l) / 2, (1 + l) / 2]
    return tuple(q)


@functools.lru_cache(maxsize=None)
def _samples(S, n, p, seed=0):
    F = np.random.default_rng(1000 * S + 10 * n + p + seed).standard_normal((S, n, p)) + 1.5
    F.setflags(write=False)
    return F


def _targets(F, bands=None, seed=0):
    """targets around the sample mean; by entry index some equal a sample (ties), some below the
    minimum / above the maximum, some NaN, and (given the bands) some equal to a band edge"""
    S, n, p = F.shape
    rng = np.random.default_rng(77 + S + n + p + seed)
    y = F.mean(0) + 0.8 * rng.standard_normal((n, p))
    e = np.arange(n * p).reshape(n, p)
    pick = rng.integers(0, S, (n, p))
    tie = np.take_along_axis(F, pick[None], 0)[0]
    y = np.where(e % 7 == 1, tie, y)
    y = np.where(e % 11 == 3, F.min(0) - 0.5, y)
    y = np.where(e % 13 == 5, F.max(0) + 0.5, y)
    if bands is not None:
        y = np.where(e % 9 == 2, bands[0], y)     # the lower edge of the first level
        y = np.where(e % 9 == 4, bands[3], y)     # the upper edge of the second level
        y = np.where(e % 9 == 6, bands[5], y)     # the upper edge of the third
    y = np.where(e % 17 == 7, np.nan, y)
    return y


def _reference(F, y, bins=BINS):
    """numpy's per-entry values: status masks, below, equal, bin, crps (long double), mean |d|"""
    S = F.shape[0]
    nan_s = np.isnan(F).any(0)
    missing = np.isnan(y)
    bad = nan_s & ~missing
    ok = ~nan_s & ~missing
    with np.errstate(invalid="ignore"):
        below = (F < y).sum(0)
        equal = (F == y).sum(0)
        x = np.sort(F, axis=0).astype(np.longdouble)
        d = x - y.astype(np.longdouble)
        w = (2 * np.arange(S) - S + 1).astype(np.longdouble).reshape((S,) + (1,) * (F.ndim - 1))
        crps = np.abs(d).sum(0) / S - (w * d).sum(0) / (np.longdouble(S) * S)
        mad = np.abs(d).mean(0).astype(np.float64)
    pbin = np.minimum(bins - 1, ((2 * below + equal) * bins) // (2 * S))
    return dict(ok=ok, missing=missing, bad=bad, below=below, equal=equal, bin=pbin, crps=crps,
                mad=mad, x=x)


def _pairwise_crps(x, y):
    """mean |x - y| - mean |x - x'| / 2 in long double, O(S^2)"""
    S = x.shape[0]
    yl = y.astype(np.longdouble)
    acc = np.zeros(x.shape[1:], dtype=np.longdouble)
    for k in range(S):
        acc += np.abs(x - x[k]).sum(0)
    return np.abs(x - yl).sum(0) / S - acc / (2 * np.longdouble(S) * S)


def _check(F, y, sc, bands, levels=LEVELS, bins=BINS):
    """a SampleScores with entries against the numpy reference; bands: sample_quantiles' rows for
    _band_levels(levels) on the same tensor"""
    if F.ndim == 2:
        F, y, bands = F[:, :, None], y[:, None], bands[:, :, None]
        ent = [np.asarray(a)[:, None] for a in (sc.crps_entries, sc.below, sc.equal)]
    else:
        ent = [np.asarray(a) for a in (sc.crps_entries, sc.below, sc.equal)]
    S, n, p = F.shape
    r = _reference(F, y, bins)
    ok = r["ok"]
    ce, be, ee = ent
    # integers: exact
    assert np.array_equal(sc.scored, ok.sum(0)) and np.array_equal(sc.missing, r["missing"].sum(0))
    assert np.array_equal(sc.bad, r["bad"].sum(0))
    assert np.array_equal(sc.scored + sc.missing + sc.bad, np.full(p, n))
    assert be.dtype == np.int32 and ee.dtype == np.int32
    assert np.array_equal(be[ok], r["below"][ok]) and np.array_equal(ee[ok], r["equal"][ok])
    assert np.all(be[~ok] == -1) and np.all(ee[~ok] == -1) and np.all(np.isnan(ce[~ok]))
    hist = np.zeros((bins, p), dtype=np.int64)
    for c in range(p):
        hist[:, c] = np.bincount(r["bin"][ok[:, c], c], minlength=bins)
    assert np.array_equal(sc.pit_hist, hist)
    gbin = np.minimum(bins - 1, ((2 * be.astype(np.int64) + ee) * bins) // (2 * S))
    assert np.array_equal(gbin[ok], r["bin"][ok])
    # inside counts: exactly the bands'
    for l in range(len(levels)):
        lo, hi = bands[2 * l], bands[2 * l + 1]
        with np.errstate(invalid="ignore"):
            inside = (lo <= y) & (y <= hi) & ok
        cnt = inside.sum(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            want = cnt / ok.sum(0).astype(np.float64)
        assert np.array_equal(sc.coverage[l], want, equal_nan=True), (S, levels[l])
    # crps per entry
    tol = 2 * (S + 4) * EPS * r["mad"]
    err = np.abs(ce.astype(np.longdouble) - r["crps"]).astype(np.float64)
    pos = ok & (tol > 0)
    worst = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    print(f"S={S} shape=({n}, {p}) worst |crps - long double| / tolerance = {worst:.4f}")
    assert np.all(err[ok] <= tol[ok]), (S, worst)
    if S == 1:
        assert np.array_equal(_bits(ce[ok]), _bits(np.abs(F[0] - y)[ok]))
    if S <= 200:
        pw = _pairwise_crps(r["x"], y)
        err2 = np.abs(ce.astype(np.longdouble) - pw).astype(np.float64)
        assert np.all(err2[ok] <= tol[ok]), (S, float((err2[ok] / np.maximum(tol[ok], 1e-300)).max()))
    # the aggregate: the mean of the per-entry values
    for c in range(p):
        k = int(ok[:, c].sum())
        if k == 0:
            assert np.isnan(sc.crps[c])
            continue
        mean = float(np.sum(ce[ok[:, c], c].astype(np.longdouble)) / k)
        assert abs(sc.crps[c] - mean) <= (n + 2) * EPS * mean, (S, c)


def _score_dev(F, y, **kw):
    import torch
    kw.setdefault("levels", LEVELS)
    kw.setdefault("bins", BINS)
    sc = G.score_samples(torch.tensor(F, device="cuda"), torch.tensor(y, device="cuda"),
                         entries=True, **kw)
    return _to_host(sc)


def _to_host(sc):
    for name in ("crps_entries", "below", "equal"):
        a = getattr(sc, name)
        if a is not None and not isinstance(a, np.ndarray):
            setattr(sc, name, a.cpu().numpy())
    return sc


def _same(a, b):
    """two SampleScores agree bit for bit, entries included"""
    for name in ("crps", "coverage"):
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    for name in ("pit_hist", "scored", "missing", "bad", "below", "equal"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(_bits(a.crps_entries), _bits(b.crps_entries))


@pytest.mark.parametrize("np_", SHAPES, ids=lambda s: f"n{s[0]}p{s[1]}")
@pytest.mark.parametrize("S", SIZES)
def test_sizes_against_numpy_on_the_expected_path(S, np_):
    import torch
    n, p = np_
    F = _samples(S, n, p)
    Fd = torch.tensor(F, device="cuda")
    bands = G.sample_quantiles(Fd, _band_levels(LEVELS)).cpu().numpy()
    y = _targets(F, bands)
    r0, l0 = _counters()
    sc = _to_host(G.score_samples(Fd, torch.tensor(y, device="cuda"), entries=True))
    r1, l1 = _counters()
    if S <= REG_MAX:
        assert r1 > r0 and l1 == l0, "the register path serves S <= 64"
    else:
        assert l1 > l0 and r1 == r0, "the LDS path serves S > 64"
    assert sc.levels == LEVELS and sc.pit_hist.shape == (BINS, p)
    assert sc.coverage.shape == (3, p)
    _check(F, y, sc, bands)
    # without entries: the same aggregates
    plain = G.score_samples(Fd, torch.tensor(y, device="cuda"))
    assert plain.crps_entries is None and plain.below is None and plain.equal is None
    assert np.array_equal(_bits(plain.crps), _bits(sc.crps))
    assert np.array_equal(plain.pit_hist, sc.pit_hist)


@pytest.mark.parametrize("S", (2, 16, 100, 129))
def test_samples_far_from_zero_and_other_options(S):
    """the centred form does not cancel at an offset of 1e4; 8 levels, 64 bins, 1 bin"""
    import torch
    F = _samples(S, 77, 3) + 1e4
    levels = (0.1, 0.25, 0.5, 0.6, 0.8, 0.9, 0.95, 0.99)
    bands = G.sample_quantiles(torch.tensor(F, device="cuda"), _band_levels(levels)).cpu().numpy()
    y = _targets(F, bands)
    _check(F, y, _score_dev(F, y, levels=levels, bins=64), bands, levels, 64)
    _check(F, y, _score_dev(F, y, levels=(0.5,), bins=1), bands[4:6], (0.5,), 1)


@pytest.mark.parametrize("S", (3, 16, 33, 100, 1000))
def test_inside_flags_agree_with_the_bands_entry_for_entry(S):
    """every entry scored on its own (n = p = 1: coverage is the flag itself), targets on the band
    edges included; and the counts bracketed by what below / equal decide on their own"""
    import torch
    n, p = 40, 3
    F = _samples(S, n, p, seed=5)
    Fd = torch.tensor(F, device="cuda")
    q = _band_levels(LEVELS)
    bands = G.sample_quantiles(Fd, q).cpu().numpy()
    y = _targets(F, bands)
    yd = torch.tensor(y, device="cuda")
    r = _reference(F, y)
    for i in range(n):
        for c in range(p):
            one = G.score_samples(Fd[:, i:i + 1, c], yd[i:i + 1, c])
            if not r["ok"][i, c]:
                assert one.scored[0] == 0 and np.all(np.isnan(one.coverage))
                continue
            for l in range(3):
                want = bands[2 * l, i, c] <= y[i, c] <= bands[2 * l + 1, i, c]
                assert one.coverage[l, 0] == float(want), (S, i, c, l)
    on_edge = sum(int(((y == bands[j]) & r["ok"]).sum()) for j in (0, 3, 5))
    assert on_edge >= 3, "some targets sit on a band edge"
    sc = _score_dev(F, y)
    ok, be, ee = r["ok"], sc.below.astype(np.int64), sc.equal.astype(np.int64)
    for l in range(3):
        (lo0, g0), (lo1, g1) = [(int(np.floor(h)), h - np.floor(h))
                                for h in (q[2 * l] * (S - 1), q[2 * l + 1] * (S - 1))]
        top = lo1 if g1 == 0 else min(lo1 + 1, S - 1)
        surely_in = ok & (be + ee >= lo0 + (1 if g0 == 0 else 2)) & (be <= lo1)
        surely_out = ok & ((be + ee <= lo0) | (be >= top + 1))
        cnt = np.rint(sc.coverage[l] * sc.scored).astype(np.int64)
        assert np.all(surely_in.sum(0) <= cnt) and np.all(cnt <= ok.sum(0) - surely_out.sum(0))


@pytest.mark.parametrize("S", (1, 2, 3, 16, 17, 33, 64))
def test_both_paths_agree_bit_for_bit(S, monkeypatch):
    F = _samples(S, 77, 3)
    y = _targets(F)
    out = {}
    for path in ("reg", "lds"):
        monkeypatch.setenv("GPAR_SCORE_PATH", path)
        r0, l0 = _counters()
        out[path] = _score_dev(F, y)
        r1, l1 = _counters()
        assert (r1 > r0, l1 > l0) == (path == "reg", path == "lds")
    _same(out["reg"], out["lds"])


def test_forcing_the_register_path_leaves_long_lists_to_lds(monkeypatch):
    F = _samples(65, 65, 1)
    y = _targets(F)
    monkeypatch.setenv("GPAR_SCORE_PATH", "reg")
    r0, l0 = _counters()
    _score_dev(F, y)
    r1, l1 = _counters()
    assert r1 == r0 and l1 > l0


def _raw_score(Fd, yd, crps_e, below_e, equal_e, levels=LEVELS, bins=BINS):
    """gpar_score_samples through ctypes, the per-entry outputs strided device views"""
    S, n, p = Fd.shape
    ctx, lib = G.context(0), G.load()
    la = np.asarray(levels, dtype=np.float64)
    crps, cov = np.empty(p), np.empty((len(levels), p))
    hist = np.zeros((bins, p), dtype=np.int64)
    cnt = [np.zeros(p, dtype=np.int64) for _ in range(3)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    with G.api._after_torch(ctx, True):
        ctx.check(lib.gpar_score_samples(
            ctx.h, S, n, p, Fd.data_ptr(), *Fd.stride(), yd.data_ptr(), *yd.stride(), len(levels),
            ptr(la), bins, G.api._lib.GPAR_MEM_DEVICE, crps_e.data_ptr(), *crps_e.stride(), below_e.data_ptr(),
            *below_e.stride(), equal_e.data_ptr(), *equal_e.stride(), ptr(crps), ptr(cov),
            ptr(hist), ptr(cnt[0]), ptr(cnt[1]), ptr(cnt[2])))
    return G.SampleScores(crps, cov, hist, cnt[0], cnt[1], cnt[2], tuple(levels),
                          crps_e.cpu().numpy(), below_e.cpu().numpy(), equal_e.cpu().numpy())


@pytest.mark.parametrize("S", (16, 100, 200))
def test_layouts_and_memory_kinds_give_the_packed_bits(S):
    import torch
    n, P = 90, 5
    F = _samples(S, n, P, seed=3)
    y = _targets(F)
    chain, yd = torch.tensor(F, device="cuda"), torch.tensor(y, device="cuda")
    score = lambda f, t: _to_host(G.score_samples(f, t, entries=True))   # noqa: E731
    packed = score(chain, yd)
    _same(packed, score(chain, yd))                                      # two identical calls

    def part(sel):
        """packed's per-entry values on a selection; its aggregates come from a packed call"""
        return [a[sel] for a in (packed.crps_entries, packed.below, packed.equal)]

    def same_as_packed_copy(f, t):
        a, b = score(f, t), score(f.contiguous(), t.contiguous())
        _same(a, b)
        return a
    # a column of the wider chain, read in place (ld_r = P), with a column of y
    col = same_as_packed_copy(chain[:, :, 2], yd[:, 2])
    assert chain[:, :, 2].stride() == (n * P, P)
    for a, b in zip((col.crps_entries, col.below, col.equal), part((slice(None), 2))):
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
    # a row block
    blk = same_as_packed_copy(chain[:, 13:71], yd[13:71])
    assert np.array_equal(_bits(blk.crps_entries), _bits(packed.crps_entries[13:71]))
    assert np.array_equal(blk.below, packed.below[13:71])
    # every other sample
    same_as_packed_copy(chain[::2], yd)
    # samples innermost (a transposed view)
    tr = chain.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert tr.stride() == (1, P * S, S)
    _same(score(tr, yd), packed)
    # strided y
    ybig = torch.full((n, 2 * P), -7.0, dtype=torch.float64, device="cuda")
    ybig[:, ::2] = yd
    _same(score(chain, ybig[:, ::2]), packed)
    # strided per-entry outputs, their neighbours untouched
    cbig = torch.full((n, 2 * P + 1), -7.0, dtype=torch.float64, device="cuda")
    bbig = torch.full((2 * n, P), -7, dtype=torch.int32, device="cuda")
    ebig = torch.full((n, P, 2), -7, dtype=torch.int32, device="cuda")
    raw = _raw_score(chain, yd, cbig[:, 1::2], bbig[::2], ebig[:, :, 1])
    _same(raw, packed)
    assert bool((cbig[:, 0::2] == -7.0).all()) and bool((bbig[1::2] == -7).all())
    assert bool((ebig[:, :, 0] == -7).all())
    # host memory: the same bits, packed and as views
    host = G.score_samples(F, y, entries=True)
    assert isinstance(host.crps_entries, np.ndarray) and host.below.dtype == np.int32
    _same(host, packed)
    _same(G.score_samples(F[:, :, 2], y[:, 2], entries=True), col)
    _same(G.score_samples(F[:, 13:71], y[13:71], entries=True), blk)


@pytest.mark.parametrize("n", (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 41))
def test_reduction_edges(n):
    import torch
    S, p = 16, 2
    F = _samples(S, n, p, seed=9)
    Fd = torch.tensor(F, device="cuda")
    bands = G.sample_quantiles(Fd, _band_levels(LEVELS)).cpu().numpy()
    y = _targets(F, bands)
    yd = torch.tensor(y, device="cuda")
    packed = _to_host(G.score_samples(Fd, yd, entries=True))
    _check(F, y, packed, bands)
    wide = torch.zeros((S, n, 2 * p + 1), dtype=torch.float64, device="cuda")
    wide[:, :, 1::2] = Fd
    ywide = torch.zeros((2 * n, p), dtype=torch.float64, device="cuda")
    ywide[::2] = yd
    _same(_to_host(G.score_samples(wide[:, :, 1::2], ywide[::2], entries=True)), packed)
    _same(G.score_samples(F, y, entries=True), packed)


@pytest.mark.parametrize("S", (3, 16, 100, 1000))
def test_nan_samples_and_targets(S):
    import torch
    n, p = 40, 3
    F = _samples(S, n, p, seed=11).copy()
    y = _targets(F)
    y[8, 0] = y[9, 1] = y[10, 2] = y[11, 1] = 1.25           # targets present where samples are NaN
    F[0, 8, 0] = np.nan                                      # first sample
    F[S // 2, 9, 1] = np.nan                                 # a middle sample
    F[S - 1, 10, 2] = np.nan                                 # the last sample
    F[:, 11, 1] = np.nan                                     # all NaN
    F[0, 12, 0], y[12, 0] = np.nan, np.nan                   # a NaN sample under a NaN target
    y[8, 1] = y[9, 2] = np.nan
    nan_s = np.isnan(F).any(0)
    assert nan_s.sum() == 5
    bands = G.sample_quantiles(torch.tensor(F, device="cuda"), _band_levels(LEVELS)).cpu().numpy()
    got = _score_dev(F, y)
    _check(F, y, got, bands)
    assert got.bad.tolist() == [1, 2, 1] and got.missing[0] >= 1
    assert got.below[12, 0] == -1 and got.below[8, 0] == -1 and np.isnan(got.crps_entries[9, 1])
    # every other entry and every aggregate: the cleaned tensor's, those targets NaN
    clean, yc = F.copy(), y.copy()
    clean[:, nan_s] = 0.0
    yc[nan_s] = np.nan
    ref = _score_dev(clean, yc)
    keep = ~nan_s
    assert np.array_equal(_bits(got.crps_entries[keep]), _bits(ref.crps_entries[keep]))
    assert np.array_equal(got.below[keep], ref.below[keep])
    assert np.array_equal(got.equal[keep], ref.equal[keep])
    for name in ("crps", "coverage"):
        assert np.array_equal(_bits(getattr(got, name)), _bits(getattr(ref, name)))
    assert np.array_equal(got.pit_hist, ref.pit_hist) and np.array_equal(got.scored, ref.scored)
    assert np.array_equal(got.missing + got.bad, ref.missing)


def test_an_output_with_nothing_scored_and_infinities():
    """NaN aggregates where no entry counts; +-inf samples and targets do not fault"""
    import torch
    F = _samples(16, 20, 2).copy()
    y = _targets(F)
    y[:, 1] = np.nan
    F[3, 4, 0], F[5, 6, 0] = np.inf, -np.inf
    y[7, 0] = np.inf
    sc = _score_dev(F, y)
    assert sc.scored[1] == 0 and sc.missing[1] == 20 and np.isnan(sc.crps[1])
    assert np.all(np.isnan(sc.coverage[:, 1])) and np.all(sc.pit_hist[:, 1] == 0)
    assert sc.scored[0] + sc.missing[0] == 20
    assert sc.below[7, 0] == 16 and sc.equal[7, 0] == 0


# ---------------------------------------------------------------------------- Gaussian scorer
def _gauss_inputs(n, p, seed=0):
    rng = np.random.default_rng(500 + n + p + seed)
    z = rng.uniform(-8.0, 8.0, (n, p))
    mean = rng.standard_normal((n, p)) * 3.0
    std = 10.0 ** rng.uniform(-1.0, 1.0, (n, p))
    y = mean + z * std
    return mean, std, y


def _ulp(x):
    return float(np.spacing(abs(x)))


def _gauss_reference(mean, std, y, levels, bins):
    """per-entry host fp64 values and which entries sit within 4 ulp of a count's boundary"""
    n, p = mean.shape
    ld, crps, se = np.empty((n, p)), np.empty((n, p)), np.empty((n, p))
    ldmag = np.empty((n, p))
    pbin = np.zeros((n, p), dtype=np.int64)
    inside = np.zeros((len(levels), n, p), dtype=bool)
    near = np.zeros((n, p), dtype=bool)
    zl = [NormalDist().inv_cdf((1 + l) / 2) for l in levels]
    for i in range(n):
        for c in range(p):
            mu, sg, t = float(mean[i, c]), float(std[i, c]), float(y[i, c])
            if math.isnan(t) or math.isnan(mu) or math.isnan(sg) or not sg > 0:
                ld[i, c] = crps[i, c] = se[i, c] = ldmag[i, c] = np.nan
                continue
            z = (t - mu) / sg
            Phi = 0.5 * math.erfc(-z / math.sqrt(2.0))
            phi = math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
            a, b = 0.5 * math.log(2.0 * math.pi * sg * sg), 0.5 * z * z
            ld[i, c], ldmag[i, c] = -a - b, abs(a) + b
            crps[i, c] = sg * (z * math.erf(z / math.sqrt(2.0)) + 2.0 * phi
                               - 1.0 / math.sqrt(math.pi))
            se[i, c] = (t - mu) ** 2
            pb = Phi * bins
            pbin[i, c] = min(bins - 1, int(math.floor(pb)))
            # (the bin is clamped to bins - 1, so only the boundaries 1 .. bins - 1 can move it)
            if 1 <= round(pb) <= bins - 1 and abs(pb - round(pb)) <= 4 * _ulp(pb):
                near[i, c] = True
            for l, q in enumerate(zl):
                inside[l, i, c] = abs(z) <= q
                if abs(abs(z) - q) <= 4 * _ulp(q):
                    near[i, c] = True
    return dict(ld=ld, ldmag=ldmag, crps=crps, se=se, bin=pbin, inside=inside, near=near)


def _check_gauss(mean, std, y, sc, levels=LEVELS, bins=BINS):
    n, p = mean.shape
    r = _gauss_reference(mean, std, y, levels, bins)
    missing = np.isnan(y)
    ok = ~np.isnan(r["crps"])
    bad = ~ok & ~missing
    assert np.array_equal(sc.scored, ok.sum(0)) and np.array_equal(sc.missing, missing.sum(0))
    assert np.array_equal(sc.bad, bad.sum(0))
    ce, le, se = (np.asarray(a).reshape(n, p) for a in
                  (sc.crps_entries, sc.log_density_entries, sc.sq_err_entries))
    for a in (ce, le, se):
        assert np.all(np.isnan(a[~ok]))
    rel = {
        "crps": np.abs(ce - r["crps"])[ok] / np.abs(r["crps"])[ok],
        # a difference of two terms: relative to the terms' magnitudes, not to what is left
        "log_density": np.abs(le - r["ld"])[ok] / r["ldmag"][ok],
        "sq_err": np.abs(se - r["se"])[ok] / np.maximum(r["se"][ok], 1e-300),
    }
    worst = {k: float(v.max()) if v.size else 0.0 for k, v in rel.items()}
    print(f"gaussian ({n}, {p}) worst relative errors: " +
          ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    # the counts: exact but for entries within 4 ulp of a boundary, which the host reference alone
    # must put below 1 %
    near = r["near"] & ok
    assert near.sum() < 0.01 * max(ok.sum(), 1) or ok.sum() < 100 and near.sum() == 0
    sure = ok & ~near
    for c in range(p):
        lower = np.bincount(r["bin"][sure[:, c], c], minlength=bins)
        extra = sc.pit_hist[:, c] - lower
        assert np.all(extra >= 0) and extra.sum() == near[:, c].sum()
        for l in range(len(levels)):
            lo = int((r["inside"][l, :, c] & sure[:, c]).sum())
            cnt = int(np.rint(sc.coverage[l, c] * sc.scored[c])) if sc.scored[c] else 0
            assert lo <= cnt <= lo + int(near[:, c].sum())
    for c in range(p):
        k = int(ok[:, c].sum())
        if k == 0:
            assert np.isnan(sc.crps[c]) and np.isnan(sc.log_density[c]) and np.isnan(sc.mse[c])
            continue
        for agg, per in ((sc.crps, ce), (sc.mse, se)):
            m = float(np.sum(per[ok[:, c], c].astype(np.longdouble)) / k)
            assert abs(agg[c] - m) <= (n + 2) * EPS * m
        v = le[ok[:, c], c].astype(np.longdouble)
        assert abs(sc.log_density[c] - float(v.sum() / k)) <= (n + 2) * EPS * float(np.abs(v).sum() / k)
    return worst


@pytest.mark.parametrize("np_", ((1, 1), (65, 1), (300, 5)), ids=lambda s: f"n{s[0]}p{s[1]}")
def test_gaussian_scores_against_the_host_evaluation(np_):
    import torch
    n, p = np_
    mean, std, y = _gauss_inputs(n, p)
    e = np.arange(n * p).reshape(n, p)
    if n > 1:
        y = np.where(e % 17 == 7, np.nan, y)
        mean = np.where(e % 19 == 4, np.nan, mean)
        std = np.where(e % 23 == 6, np.nan, std)
        std = np.where(e % 29 == 9, 0.0, std)
        std = np.where(e % 31 == 11, -1.0, std)
    dev = [torch.tensor(a, device="cuda") for a in (mean, std, y)]
    sc = G.score_gaussian(*dev, entries=True)
    for name in ("crps_entries", "log_density_entries", "sq_err_entries"):
        setattr(sc, name, getattr(sc, name).cpu().numpy())
    worst = _check_gauss(mean, std, y, sc)
    assert max(worst.values()) <= GAUSS_RTOL, worst
    # strided views and host memory: the same bits
    wide = torch.zeros((3, n, 2 * p), dtype=torch.float64, device="cuda")
    for k in range(3):
        wide[k, :, 1::2] = dev[k]
    sv = G.score_gaussian(wide[0, :, 1::2], wide[1, :, 1::2], wide[2, :, 1::2], entries=True)
    sh = G.score_gaussian(mean, std, y, entries=True)
    for other in (sv, sh):
        for name in ("crps", "log_density", "mse", "coverage"):
            assert np.array_equal(_bits(getattr(other, name)), _bits(getattr(sc, name))), name
        for name in ("pit_hist", "scored", "missing", "bad"):
            assert np.array_equal(getattr(other, name), getattr(sc, name)), name
        for name in ("crps_entries", "log_density_entries", "sq_err_entries"):
            a = getattr(other, name)
            a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
            assert np.array_equal(_bits(a), _bits(getattr(sc, name))), name
    # one-dimensional inputs
    if p == 1:
        s1 = G.score_gaussian(dev[0][:, 0], dev[1][:, 0], dev[2][:, 0], entries=True)
        assert tuple(s1.crps_entries.shape) == (n,)
        assert np.array_equal(_bits(s1.crps), _bits(sc.crps))


def test_ensemble_crps_approaches_the_gaussian_crps():
    """S = 4096 Gaussian draws per entry: the two CRPS agree within 5 sigma / sqrt(S), the project's
    rule for Monte-Carlo estimates against their analytic limit"""
    import torch
    S, n, p = 4096, 24, 2
    mean, std, y = _gauss_inputs(n, p, seed=3)
    y = mean + np.clip((y - mean) / std, -3.0, 3.0) * std
    F = mean + std * np.random.default_rng(12).standard_normal((S, n, p))
    ens = _score_dev(F, y)
    gs = G.score_gaussian(torch.tensor(mean, device="cuda"), torch.tensor(std, device="cuda"),
                          torch.tensor(y, device="cuda"), entries=True)
    diff = np.abs(ens.crps_entries - gs.crps_entries.cpu().numpy())
    print(f"ensemble vs gaussian crps: worst |diff| / (5 sigma / sqrt S) = "
          f"{float((diff / (5 * std / math.sqrt(S))).max()):.3f}")
    assert np.all(diff <= 5 * std / math.sqrt(S))


# ---------------------------------------------------------------------------- errors, end to end
def test_errors_launch_nothing():
    import torch
    F = _samples(16, 64, 1)
    y = _targets(F)
    Fd, yd = torch.tensor(F, device="cuda"), torch.tensor(y, device="cuda")
    ctx = G.context(0)
    G.score_samples(Fd, yd)
    c0 = _counters()
    with pytest.raises(G.Unsupported):
        G.score_samples(torch.zeros((4097, 3), dtype=torch.float64, device="cuda"),
                        torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(G.Unsupported):
        G.score_samples(np.zeros((4097, 3)), np.zeros(3))
    for levels in ((0.0,), (1.0,), (float("nan"),), (0.5, 1.5), tuple(0.1 * k for k in range(1, 10))):
        for args in ((Fd, yd), (F, y)):
            with pytest.raises(G.DomainError):
                G.score_samples(*args, levels=levels)
            with pytest.raises(G.DomainError):
                G.score_gaussian(args[0][0], args[0][1] ** 2 + 1.0, args[1], levels=levels)
    for bins in (0, 65, -1):
        for args in ((Fd, yd), (F, y)):
            with pytest.raises(G.DomainError):
                G.score_samples(*args, bins=bins)
            with pytest.raises(G.DomainError):
                G.score_gaussian(args[0][0], args[0][1] ** 2 + 1.0, args[1], bins=bins)
    # strides under which two entries share an address: F, then y
    flat = torch.arange(4096, dtype=torch.float64, device="cuda")
    y2 = torch.zeros((64, 2), dtype=torch.float64, device="cuda")
    for size, stride in (((16, 64, 2), (64, 1, 1)), ((16, 64, 2), (32, 2, 1)),
                         ((16, 64, 2), (128, 2, 2))):
        with pytest.raises(G.DomainError):
            G.score_samples(torch.as_strided(flat, size, stride), y2)
    with pytest.raises(G.DomainError):
        G.score_samples(torch.as_strided(flat, (16, 64), (1, 1)), y2[:, 0])
    with pytest.raises(G.DomainError):
        G.score_samples(torch.as_strided(flat, (16, 64, 2), (128, 2, 1)),
                        torch.as_strided(flat, (64, 2), (1, 1)))
    hflat = np.arange(4096.0)
    with pytest.raises(G.DomainError):
        G.score_samples(np.lib.stride_tricks.as_strided(hflat, (16, 64, 2), (512, 8, 8)),
                        np.zeros((64, 2)))
    # a y of the wrong shape
    for bad_y in (yd[:63], yd[:, 0], torch.zeros((64, 2), dtype=torch.float64, device="cuda")):
        with pytest.raises(G.DomainError):
            G.score_samples(Fd, bad_y)
    with pytest.raises(G.DomainError):
        G.score_samples(Fd, y)                      # a host y for device samples
    assert _counters() == c0
    # an admissible interleaving is not an alias: rows of two columns, columns 64 apart
    ok = torch.as_strided(flat, (16, 64, 2), (128, 1, 64))
    a, b = G.score_samples(ok, y2), G.score_samples(ok.contiguous(), y2)
    assert np.array_equal(_bits(a.crps), _bits(b.crps)) and np.array_equal(a.pit_hist, b.pit_hist)
    assert ctx.workspace_bytes() > 0


@functools.lru_cache(maxsize=None)
def _posterior():
    """three outputs in the GPAR ordering on the device (test_gpu_quantiles.py's builder: n = 300,
    M = 32, N* = 50): output i reads the given column and outputs 0..i-1"""
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
    held_out = np.stack([np.interp(ts, t, Y[:, 1 + i]) for i in range(3)], axis=1)
    held_out[::7, 1] = np.nan
    return post, tsd, given, torch.from_numpy(held_out).cuda()


def test_sample_chain_scores_end_to_end():
    import torch
    post, tsd, given, y_star = _posterior()
    S = 16
    plain = post.sample_chain(tsd, given, S, seed=40)
    chain, means, stds, sc = post.sample_chain_scores(tsd, given, S, y_star, seed=40)
    assert torch.equal(chain, plain[0])
    for a, b in zip(means + stds, plain[1] + plain[2]):
        assert torch.equal(a, b)
    ref = G.score_samples(chain, y_star)
    for name in ("crps", "coverage"):
        assert np.array_equal(_bits(getattr(sc, name)), _bits(getattr(ref, name)))
    for name in ("pit_hist", "scored", "missing", "bad"):
        assert np.array_equal(getattr(sc, name), getattr(ref, name))
    assert np.array_equal(sc.scored + sc.missing + sc.bad, np.full(3, 50))
    assert sc.missing.tolist() == [0, 8, 0] and np.all(sc.crps > 0)
    bands = G.sample_quantiles(chain, _band_levels(LEVELS)).cpu().numpy()
    _check(chain.cpu().numpy(), y_star.cpu().numpy(),
           _to_host(G.score_samples(chain, y_star, entries=True)), bands)
    other = post.sample_chain_scores(tsd, given, S, y_star, levels=(0.8,), bins=4, seed=40)[3]
    assert other.coverage.shape == (1, 3) and other.pit_hist.shape == (4, 3)
    assert other.levels == (0.8,) and np.array_equal(_bits(other.crps), _bits(sc.crps))


def test_device_call_keeps_the_workspace_and_reports_its_bytes():
    import torch
    S, n, p = 100, 300, 5
    F = _samples(S, n, p)
    Fd, yd = torch.tensor(F, device="cuda"), torch.tensor(_targets(F), device="cuda")
    ctx = G.context(0)
    G.score_samples(Fd, yd, entries=True)
    before = ctx.workspace_bytes()
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        G.score_samples(Fd, yd, entries=True)
        launches, ms = ctx.kernel_stats("score")
        assert launches == 1 and ms > 0.0
        assert ctx.kernel_work("score") == 8.0 * S * n * p
    finally:
        ctx.set_profiling(False)
    assert ctx.workspace_bytes() == before
