"""Pseudo-input selection on the device (gpar_select_pseudo_inputs, k_kmeans.hip) against a numpy
restatement of Lloyd's k-means with exact differences ((V[:, None] - Z[None]) ** 2).sum(-1).

Inputs: gpar_dataset(3001, 72, seed=3), V = Y[:, :D] read in place (ldv = 72), Z0 =
pseudo_inputs(V, M, 11), at (D, M) = (1, 5), (3, 130), (17, 300), (70, 130), (64, 257) and one
case of n = 37, D = 3, M = 5: n off the 128-row tile and below one tile, D below / at / above one
16-wide K-step and at / above 64, M below and across 128 and 256.

The assignment tolerance is the bound of a D-term fp64 dot product in the centred Gram form,
tol_k = 4 (D + 8) eps (|v_k - g|^2 + max_c |z_c - g|^2), g the column mean of V.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gparatscale")
from gparatscale import _lib as L  # noqa: E402
from gparatscale import data as Dd  # noqa: E402

EPS = np.finfo(np.float64).eps
N, P = 3001, 72
SHAPES = [(N, 1, 5), (N, 3, 130), (N, 17, 300), (N, 70, 130), (N, 64, 257), (37, 3, 5)]
IDS = [f"n{n}_D{d}_M{m}" for n, d, m in SHAPES]


@functools.lru_cache(maxsize=None)
def _data():
    ds = Dd.gpar_dataset(N, P, seed=3)
    Y = np.ascontiguousarray(ds["Y"])
    Y.setflags(write=False)
    return ds["t"], Y


@functools.lru_cache(maxsize=None)
def _inputs(n, d, m):
    """V: an n x d view into the n x 72 outputs (ldv = 72), Z0: m of its rows."""
    _, Y = _data()
    V = Y[:n, :d]
    Z0 = Dd.pseudo_inputs(V, m, 11)
    Z0.setflags(write=False)
    return V, Z0


def _d2_ref(V, Z):
    """((V[:, None] - Z[None]) ** 2).sum(-1), evaluated in row blocks (the same numbers)."""
    out = np.empty((V.shape[0], Z.shape[0]))
    for k0 in range(0, V.shape[0], 256):
        out[k0:k0 + 256] = ((V[k0:k0 + 256, None] - Z[None]) ** 2).sum(-1)
    return out


def _tol(V, Z):
    g = V.mean(0)
    return 4.0 * (V.shape[1] + 8) * EPS * (((V - g) ** 2).sum(1) + ((Z - g) ** 2).sum(1).max())


def _select(V, Z0, iters, snap, mem="host", z_alias=False):
    """gpar_select_pseudo_inputs through ctypes, V and Z0 with their own row strides."""
    lib, ctx = L.load(), G.context(0)
    n, d = V.shape
    m = Z0.shape[0]
    inertia = np.zeros(iters + 1)
    if mem == "device":
        import torch
        _, Y = _data()
        Yd = torch.from_numpy(np.array(Y)).cuda()
        Vd = Yd[:n, :d]
        assert Vd.stride(0) == P
        Zd = torch.from_numpy(np.array(Z0)).cuda()
        zo = Zd if z_alias else torch.empty((m, d), dtype=torch.float64, device="cuda")
        idx = torch.empty(m, dtype=torch.int64, device="cuda")
        lab = torch.empty(n, dtype=torch.int32, device="cuda")
        cnt = torch.empty(m, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(lib.gpar_select_pseudo_inputs(
            ctx.h, n, d, C.c_void_p(Vd.data_ptr()), Vd.stride(0), m, C.c_void_p(Zd.data_ptr()), d,
            iters, snap, L.GPAR_MEM_DEVICE, C.c_void_p(zo.data_ptr()), d,
            C.c_void_p(idx.data_ptr()), C.c_void_p(lab.data_ptr()), C.c_void_p(cnt.data_ptr()),
            inertia.ctypes.data_as(C.c_void_p)))
        return dict(z=zo.cpu().numpy(), index=idx.cpu().numpy(), label=lab.cpu().numpy(),
                    count=cnt.cpu().numpy(), inertia=inertia)
    assert V.strides[1] == 8
    Zc = np.array(Z0)
    zo = Zc if z_alias else np.zeros((m, d))
    idx = np.zeros(m, dtype=np.int64)
    lab = np.zeros(n, dtype=np.int32)
    cnt = np.zeros(m, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx.check(lib.gpar_select_pseudo_inputs(
        ctx.h, n, d, C.c_void_p(V.ctypes.data), V.strides[0] // 8, m, p(Zc), d, iters, snap,
        L.GPAR_MEM_HOST, p(zo), d, p(idx), p(lab), p(cnt), p(inertia)))
    return dict(z=zo, index=idx, label=lab, count=cnt, inertia=inertia)


@functools.lru_cache(maxsize=None)
def _assign0(n, d, m):
    """The iters = 0, snap = 0 call on Z0 (shared by the checks that start from it)."""
    V, Z0 = _inputs(n, d, m)
    return _select(V, Z0, 0, 0)


# ------------------------------------------------------------------ 1. assignment
@pytest.mark.parametrize("n,d,m", SHAPES, ids=IDS)
def test_assignment_is_optimal_within_rounding(n, d, m):
    V, Z0 = _inputs(n, d, m)
    r = _assign0(n, d, m)
    d2 = _d2_ref(V, Z0)
    tol = _tol(V, Z0)
    lab = r["label"].astype(np.int64)
    assert lab.min() >= 0 and lab.max() < m
    chosen = d2[np.arange(n), lab]
    best = d2.min(1)
    excess = chosen - best
    part = np.partition(d2, 1, axis=1)
    margin = part[:, 1] - part[:, 0]          # second-best minus best
    share = float((margin < tol).mean())
    print(f"assign n={n} D={d} M={m}: max excess/tol {np.max(excess / tol):.3e}, "
          f"near-tie share {share:.4f}, mismatches {(lab != d2.argmin(1)).sum()}")
    assert np.all(excess <= tol)
    assert share <= 0.01          # the optimality check above is not vacuous
    np.testing.assert_array_equal(r["count"], np.bincount(lab, minlength=m))
    np.testing.assert_allclose(r["inertia"][0], chosen.sum(), rtol=1e-12)
    np.testing.assert_array_equal(r["z"], Z0)          # iters = 0, snap = 0: the centres as given
    np.testing.assert_array_equal(r["index"], -np.ones(m, dtype=np.int64))


# ------------------------------------------------------------------ 2. update
@pytest.mark.parametrize("n,d,m", SHAPES, ids=IDS)
def test_update_is_the_members_mean(n, d, m):
    V, Z0 = _inputs(n, d, m)
    prev = _assign0(n, d, m)["label"]
    r = _select(V, Z0, 1, 0)
    full = np.bincount(prev, minlength=m) > 0
    assert full.sum() >= m - 1          # Z0 are rows of V: (almost) every centre owns itself
    # the members' mean, summed in extended precision: the reference's own rounding stays far
    # below the rtol even where a mean comes out near zero
    ref = np.array(Z0, dtype=np.longdouble)
    for c in np.flatnonzero(full):
        ref[c] = np.asarray(V[prev == c], dtype=np.longdouble).mean(0)
    err = np.abs(r["z"] - ref) / np.abs(ref)
    print(f"update n={n} D={d} M={m}: max rel err {float(err.max()):.3e}")
    np.testing.assert_allclose(r["z"], ref.astype(np.float64), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(r["z"][~full], Z0[~full])


# ------------------------------------------------------------------ 3. inertia
@pytest.mark.parametrize("n,d,m", SHAPES, ids=IDS)
def test_inertia_does_not_rise(n, d, m):
    V, Z0 = _inputs(n, d, m)
    it = _select(V, Z0, 6, 0)["inertia"]
    print(f"inertia n={n} D={d} M={m}: {it}")
    assert it.shape == (7,) and np.all(np.isfinite(it))
    assert np.all(it[1:] <= it[:-1] * (1 + 1e-12))


# ------------------------------------------------------------------ 4. determinism, composition
@pytest.mark.parametrize("n,d,m", SHAPES, ids=IDS)
def test_deterministic_in_either_memory_space_and_composable(n, d, m):
    V, Z0 = _inputs(n, d, m)
    a = _select(V, Z0, 4, 0)
    b = _select(V, Z0, 4, 0)
    c = _select(V, Z0, 4, 0, mem="device")
    z, inertia = np.array(Z0), []
    for _ in range(4):
        s = _select(V, z, 1, 0, z_alias=True)          # z_out aliases z0
        z = s["z"]
        inertia.append(s["inertia"])
    chained = dict(z=z, label=s["label"], count=s["count"],
                   inertia=np.array([i[0] for i in inertia] + [inertia[-1][1]]))
    for i in range(3):
        np.testing.assert_array_equal(inertia[i][1], inertia[i + 1][0])
    for other in (b, c, chained):
        for k in ("z", "label", "inertia", "count"):
            np.testing.assert_array_equal(a[k], other[k], err_msg=k)


# ------------------------------------------------------------------ 5. edge rules
@pytest.mark.parametrize("snap", [0, 1])
def test_duplicate_and_far_centres_stay_empty_and_unchanged(snap):
    """Row 7 duplicates row 3 (the lower index takes every tie), row 1 sits at +1e3 in every
    dimension: both clusters are empty, keep their centres bit for bit and get index -1.  Centre 7
    stops being a duplicate once the first update has moved centre 3 (it then sits on the data row
    Z0[3] and takes that row back), so past the first round the rule is checked as what it is: a
    centre whose cluster was empty in every update round comes back bit-identical."""
    V, Z0 = _inputs(N, 3, 130)
    Z = np.array(Z0)
    Z[7] = Z[3]
    Z[1] = 1e3
    r0 = _select(V, Z, 0, snap)
    assert r0["count"][7] == 0 and r0["count"][1] == 0 and r0["count"][3] > 0
    np.testing.assert_array_equal(r0["z"][[1, 7]], Z[[1, 7]])
    assert r0["index"][7] == -1 and r0["index"][1] == -1
    r1 = _select(V, Z, 1, snap)
    np.testing.assert_array_equal(r1["z"][1], Z[1])
    if not snap:          # one update with cluster 7 empty (snapped, it is a row of its new members)
        np.testing.assert_array_equal(r1["z"][7], Z[7])
    r = _select(V, Z, 2, snap)
    never = (r0["count"] == 0) & (r1["count"] == 0)          # empty in both update rounds
    assert never[1] and r["count"][1] == 0
    empty = r["count"] == 0
    kept = never & empty if snap else never          # (a snap moves a cluster that has filled since)
    np.testing.assert_array_equal(r["z"][kept], Z[kept])
    assert np.all(r["index"][empty] == -1)
    if snap:
        assert np.all(r["index"][~empty] >= 0)
    else:
        assert np.all(r["index"] == -1)


# ------------------------------------------------------------------ 6. snap
@pytest.mark.parametrize("n,d,m", SHAPES, ids=IDS)
def test_snap_takes_each_clusters_nearest_member(n, d, m):
    V, Z0 = _inputs(n, d, m)
    free = _select(V, Z0, 3, 0)          # the centroids the snap starts from (same bits)
    r = _select(V, Z0, 3, 1)
    np.testing.assert_array_equal(r["label"], free["label"])
    np.testing.assert_array_equal(r["count"], free["count"])
    tol = _tol(V, free["z"])
    full = np.flatnonzero(r["count"] > 0)
    assert len(full) > 0
    idx = r["index"]
    assert np.all(idx[r["count"] == 0] == -1)
    for c in full:
        k = idx[c]
        assert 0 <= k < n
        np.testing.assert_array_equal(r["z"][c], V[k])
        assert r["label"][k] == c
        members = np.flatnonzero(r["label"] == c)
        dref = ((V[members] - free["z"][c]) ** 2).sum(-1)
        assert ((V[k] - free["z"][c]) ** 2).sum() - dref.min() <= tol[k]
    assert len(np.unique(idx[full])) == len(full)
    np.testing.assert_array_equal(r["z"][r["count"] == 0], free["z"][r["count"] == 0])


# ------------------------------------------------------------------ 7. separation
def _min_sep(Z):
    d2 = ((Z[:, None] - Z[None]) ** 2).sum(-1)
    d2[np.diag_indices_from(d2)] = np.inf
    return float(np.sqrt(d2.min()))


@pytest.mark.parametrize("d,m", [(1, 256), (3, 64)])
def test_kmeans_spreads_the_centres(d, m):
    Y = Dd.gpar_dataset(20000, 6, seed=1)["Y"]
    V = Y[:, :d]
    Z0 = Dd.pseudo_inputs(V, m, 7)
    r = _select(V, Z0, 10, 0)
    s0, s1 = _min_sep(Z0), _min_sep(r["z"])
    print(f"separation D={d} M={m}: random rows {s0:.3e}, after k-means {s1:.3e}")
    assert s1 >= s0


# ------------------------------------------------------------------ 8. end to end
THETA = (1.3, 0.9, 0.7, 1.1, 0.2)


def test_selected_pseudo_inputs_feed_the_objective():
    from oracle import gpar_oracle as O
    t, Y = _data()
    V, Z0 = _inputs(N, 3, 130)
    y = Y[:, 3]
    sel = G.select_pseudo_inputs(V.T, Z0.T, iters=10, snap=True)
    assert sel.Z.shape == (3, 130) and sel.inertia.shape == (11,)
    np.testing.assert_array_equal(sel.Z.T, V[sel.index])
    assert len(np.unique(sel.index)) == 130
    ref, _ = O.compute_gpar_dtc_objective(V.T, sel.Z, t, y, THETA)
    got = G.compute_gpar_dtc_objective(V.T, sel.Z, t, y, THETA)
    assert abs(got - ref) <= 1e-10 * max(1.0, abs(ref)), (got, ref)

    # the same on device tensors: Z goes on as a device tensor, no host copy in between
    import torch
    Yd = torch.from_numpy(np.array(Y)).cuda()
    Vd = Yd[:, :3]
    seld = G.select_pseudo_inputs(Vd, torch.from_numpy(np.array(Z0)).cuda(), iters=10, snap=True)
    assert seld.Z.is_cuda and seld.labels.is_cuda and seld.index.is_cuda
    np.testing.assert_array_equal(seld.Z.cpu().numpy(), sel.Z.T)
    np.testing.assert_array_equal(seld.index.cpu().numpy(), sel.index)
    td = torch.from_numpy(np.array(t)).cuda()
    gotd = G.compute_gpar_dtc_objective(Vd, seld.Z, td, Yd[:, 3], THETA)
    assert abs(gotd - ref) <= 1e-10 * max(1.0, abs(ref)), (gotd, ref)


def test_integer_m_draws_the_start_rows():
    V, _ = _inputs(N, 3, 130)
    a = G.select_pseudo_inputs(V.T, 130, iters=2, snap=False, seed=11)
    Z0 = V[Dd.pseudo_index(N, 130, 11)]
    b = _select(V, Z0, 2, 0)
    np.testing.assert_array_equal(a.Z.T, b["z"])
    np.testing.assert_array_equal(a.labels, b["label"])
    np.testing.assert_array_equal(a.counts, b["count"])
    np.testing.assert_array_equal(a.inertia, b["inertia"])
    assert np.all(a.index == -1)


# ------------------------------------------------------------------ 9. arguments
def _raw(ctx, n, d, v, ldv, m, z0, ldz0, iters, snap, mem, zo, ldzo):
    return L.load().gpar_select_pseudo_inputs(ctx.h, n, d, v, ldv, m, z0, ldz0, iters, snap, mem,
                                              zo, ldzo, None, None, None, None)


def test_bad_arguments_raise_and_leave_the_context_usable():
    V, Z0 = _inputs(37, 3, 5)
    Vc, Zc, zo = np.ascontiguousarray(V), np.array(Z0), np.zeros((5, 3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx = G.context(0)
    good = dict(n=37, d=3, v=p(Vc), ldv=3, m=5, z0=p(Zc), ldz0=3, iters=1, snap=1,
                mem=L.GPAR_MEM_HOST, zo=p(zo), ldzo=3)
    bad = [dict(n=0), dict(d=0), dict(m=0), dict(m=38), dict(ldv=2), dict(ldz0=2), dict(ldzo=2),
           dict(iters=-1), dict(v=None), dict(z0=None), dict(zo=None), dict(mem=2), dict(mem=-1)]
    for change in bad:
        with pytest.raises(G.GparError) as e:
            ctx.check(_raw(ctx, **{**good, **change}))
        assert e.value.code == L.GPAR_ERR_ARG, change
        assert "gpar_select_pseudo_inputs" in str(e.value), change
        ctx.check(_raw(ctx, **good))          # the context still serves a valid call
    ref = _select(V, Z0, 1, 1)
    np.testing.assert_array_equal(zo, ref["z"])
    with pytest.raises(G.DomainError):
        G.select_pseudo_inputs(V.T, 38)
    with pytest.raises(G.DomainError):
        G.select_pseudo_inputs(V.T, Z0[:, :2].T)


def test_profiling_counts_the_assignment_passes():
    V, Z0 = _inputs(N, 17, 300)
    ctx = G.context(0)
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        _select(V, Z0, 3, 1)
        launches, ms = ctx.kernel_stats("kmeans")
        work = ctx.kernel_work("kmeans")
    finally:
        ctx.set_profiling(False)
        ctx.reset_stats()
    assert launches == 4 and ms > 0.0
    assert work == 4 * 2.0 * N * 300 * 17
