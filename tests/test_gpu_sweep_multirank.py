"""GPU, two ranks on one card (gloo process group, as test_gpu_multirank): the
parameter sweep over song shards — one MAX all-reduce of every parameter's
(-min, max), one SUM all-reduce of the class-count block (through the host),
the fold on the device — gives the single-context sweep on every rank, bit
for bit."""
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp
from helpers import pg_init_method

pytestmark = pytest.mark.gpu

PARAMS = [0.9, 0.0, 0.25, 0.5, 1.0]  # a full group and a short one


def _dataset():
    from musicrecommendation_amd import synth
    return synth.config("c2", n_test=16).dataset()


def _worker(rank, world, init, out):
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        from musicrecommendation_amd import evaluation
        from musicrecommendation_amd.engine import Engine
        from musicrecommendation_amd.ensemble import DeviceEnsemble
        from musicrecommendation_amd.sharding import song_shards

        ds = _dataset()
        lo, hi = song_shards(ds, world)[rank]
        with Engine(ds, out_dtype="f64", topk=10, song_lo=lo, song_hi=hi) as e:
            ens = DeviceEnsemble(e, pos=evaluation.label_pos(ds), n_label_songs=ds.n_label_songs)
            u, i = ens.model("ubm"), ens.model("ibm")
            out[rank] = {"linear": ens.sweep("linear", u, i, PARAMS),
                         "stochastic": ens.sweep("stochastic", u, i, PARAMS, seed=2)}
    finally:
        dist.destroy_process_group()


def test_two_ranks_sweep_song_shards_on_one_gpu():
    from musicrecommendation_amd.engine import Engine
    from musicrecommendation_amd.ensemble import DeviceEnsemble

    world = 2
    ctx = mp.get_context("spawn")
    with ctx.Manager() as m:
        out = m.dict()
        mp.start_processes(_worker, args=(world, pg_init_method(), out), nprocs=world, join=True, start_method="spawn")
        res = dict(out)
    ds = _dataset()
    with Engine(ds, out_dtype="f64", topk=10) as e:
        ens = DeviceEnsemble(e)
        u, i = ens.model("ubm"), ens.model("ibm")
        full = {"linear": ens.sweep("linear", u, i, PARAMS), "stochastic": ens.sweep("stochastic", u, i, PARAMS, seed=2)}
        assert len(set(full["linear"])) > 1  # not a constant
    for r in range(world):
        assert res[r] == full, r
