"""CPU, gloo worlds of 2 and 3: the chained sweeps of gparatscale.shard with a mean_fn.

Only means travel along the chain (GPAR_scaled_examples.jl:172, eeg.jl:249,274), so with mean_fn
the ordered part of chained_predictions / chained_sweep_blocks calls it alone and the rank's
predict_fn calls, which supply the stds, run after the last broadcast / once the block's sends are
posted.  Deterministic fake workers that log their calls stand in for the GPU predictions.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

P, NS = 7, 40


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _mean(p, c):
    """A mean that depends on every earlier column of the chain, so a stale column shows."""
    c = np.asarray(c)[:, : p - 1]
    return np.sin(c @ np.arange(1.0, p)) + 0.1 * p


def _std(p, c):
    return 1.0 + np.cos(np.asarray(c)[:, : p - 1].sum(axis=1) * p) ** 2


def _first_column():
    return np.linspace(-1.0, 1.0, NS) ** 3 + 0.25


def _serial_chain():
    chain = _first_column()[:, None]
    for p in range(2, P + 1):
        chain = np.column_stack([chain, _mean(p, chain)])
    return chain


def _worker(rank, world, port, out, kind, with_mean):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "gpar-at-scale_amd", "python"))
    from gparatscale import shard as S
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real_isend, real_bcast = dist.isend, dist.broadcast

    def isend(tensor, dst, *a, **kw):
        calls.append(("isend", dst))
        return real_isend(tensor, dst, *a, **kw)

    def bcast(tensor, src, *a, **kw):
        calls.append(("broadcast", src))
        return real_bcast(tensor, src, *a, **kw)

    dist.isend, dist.broadcast = isend, bcast
    try:
        chain = torch.zeros((NS, P), dtype=torch.float64)
        chain[:, 0] = torch.from_numpy(_first_column())

        def mean_fn(p, c):
            calls.append(("mean", p))
            # inputs of p: every earlier column must already hold its mean
            assert np.all(c[:, : p - 1].numpy() != 0.0)
            return _mean(p, c.numpy())

        def predict_fn(p, c):
            calls.append(("predict", p))
            assert np.all(c[:, : p - 1].numpy() != 0.0)
            # its own mean is marked: the pairs must carry mean_fn's when there is one
            return _mean(p, c.numpy()) + (7.0 if with_mean else 0.0), _std(p, c.numpy())

        kw = dict(prepare_fn=lambda p: calls.append(("prepare", p)))
        if with_mean:
            kw["mean_fn"] = mean_fn
        if kind == "blocks":
            shards = S.assign_chained(P, world)
            own = [p for p in shards[rank] if p >= 2]
            mine = S.chained_sweep_blocks(shards, predict_fn, chain, **kw)
        else:
            owners = S.owners_of(S.assign_outputs(P, world))
            own = [p for p in range(2, P + 1) if owners[p] == rank]
            mine = S.chained_predictions(range(2, P + 1), owners, predict_fn, chain, **kw)
        ref = _serial_chain()
        assert sorted(mine) == own
        for p in own:   # (mean_fn's mean, predict_fn's std), the std against the finished inputs
            np.testing.assert_array_equal(np.asarray(mine[p][0]), ref[:, p - 1])
            np.testing.assert_array_equal(np.asarray(mine[p][1]), _std(p, ref))
        kinds = [k for k, _ in calls]
        assert [p for k, p in calls if k == "prepare"] == own
        assert [p for k, p in calls if k == "predict"] == own
        if with_mean:
            assert [p for k, p in calls if k == "mean"] == own
            if own:
                first = kinds.index("predict")
                assert "mean" not in kinds[first:]
                if kind == "blocks":   # the block's sends are posted before the stds start
                    sends = [i for i, k in enumerate(kinds) if k == "isend"]
                    assert len(sends) == world - 1 - rank and all(i < first for i in sends)
                else:                  # every output's broadcast has happened
                    casts = [i for i, k in enumerate(kinds) if k == "broadcast"]
                    assert len(casts) == P - 1 and all(i < first for i in casts)
                # each output prepared before its mean, the next one before the current mean
                for i, p in enumerate(own):
                    pos = calls.index(("mean", p))
                    assert calls.index(("prepare", p)) < pos
                    if i + 1 < len(own):
                        assert calls.index(("prepare", own[i + 1])) < pos
        else:   # today's log: prepare(first), then per output prepare(next), predict
            want = [("prepare", own[0])] if own else []
            for i, p in enumerate(own):
                if i + 1 < len(own):
                    want.append(("prepare", own[i + 1]))
                want.append(("predict", p))
            assert [c for c in calls if c[0] in ("prepare", "predict", "mean")] == want
        np.save(out + f".{rank}.npy", chain.numpy())
    finally:
        dist.isend, dist.broadcast = real_isend, real_bcast
        dist.destroy_process_group()


@pytest.mark.parametrize("with_mean", [True, False], ids=["mean_fn", "no_mean_fn"])
@pytest.mark.parametrize("kind", ["blocks", "broadcast"])
@pytest.mark.parametrize("world", [2, 3])
def test_chained_sweeps_with_mean_fn(tmp_path, world, kind, with_mean):
    """Every rank ends with the serial reference chain, bit for bit; the ordering and the returned
    pairs are asserted inside the workers."""
    out = str(tmp_path / "chain")
    mp.start_processes(_worker, args=(world, _free_port(), out, kind, with_mean), nprocs=world,
                       join=True, start_method="spawn")
    ref = _serial_chain()
    for r in range(world):
        np.testing.assert_array_equal(np.load(out + f".{r}.npy"), ref)


def test_mean_fn_on_one_process():
    """No process group: the same contract (the GPU tests run the sweeps this way)."""
    from gparatscale import shard as S
    ref = _serial_chain()
    for kind in ("blocks", "broadcast"):
        chain = torch.zeros((NS, P), dtype=torch.float64)
        chain[:, 0] = torch.from_numpy(_first_column())
        calls = []

        def mean_fn(p, c):
            calls.append(("mean", p))
            return _mean(p, c.numpy())

        def predict_fn(p, c):
            calls.append(("predict", p))
            return _mean(p, c.numpy()) + 7.0, _std(p, c.numpy())

        if kind == "blocks":
            mine = S.chained_sweep_blocks([list(range(1, P + 1))], predict_fn, chain, mean_fn=mean_fn)
        else:
            mine = S.chained_predictions(range(2, P + 1), {p: 0 for p in range(2, P + 1)},
                                         predict_fn, chain, mean_fn=mean_fn)
        np.testing.assert_array_equal(chain.numpy(), ref)
        assert calls == [("mean", p) for p in range(2, P + 1)] + [("predict", p) for p in range(2, P + 1)]
        for p in range(2, P + 1):
            np.testing.assert_array_equal(mine[p][0], ref[:, p - 1])
            np.testing.assert_array_equal(mine[p][1], _std(p, ref))
