"""GPU: the parameter sweep (mr_sweep_*: the threshold mAP of one combination
kind at P parameter values, no combined model materialised) against
* the host restatement: helpers.reference_combination over the engine's own
  ubm / ibm, cast to the model dtype, then evaluation.threshold_map /
  threshold_counts — bit for bit;
* the materialised device path: ens.linear / aggregation / stochastic +
  ens.threshold_map per value — bit for bit;
over full and short parameter groups, song shards and user blocks, scores at
the exact level boundaries, a degenerate range, the argument errors, the
driver's --sweep and the MusicRecommender mirror."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

from musicrecommendation_amd import _lib, driver, evaluation, synth
from musicrecommendation_amd.engine import Engine
from musicrecommendation_amd.ensemble import DeviceEnsemble, pair_uniform
from musicrecommendation_amd.recommender import MusicRecommender
from musicrecommendation_amd.sharding import song_shards

from helpers import dataset_from_lines, kat, pair_index, reference_combination, synth_fixture

pytestmark = pytest.mark.gpu

PARAMS = [0.0, 0.1, 0.25, 0.5, 0.5, 0.9, 1.0, 0.75]  # unsorted, a duplicate, P = 8: two full groups of 4
KINDS = ("linear", "aggregation", "stochastic")
SEED = 3
THS = {10: evaluation.THRESHOLDS, 11: evaluation.THRESHOLDS_DISTRIBUTED}


@functools.lru_cache(maxsize=None)
def dataset(name):
    if name == "kat":
        K = kat()
        return dataset_from_lines(K["train"], K["test"], K["labels"])
    if name == "small":
        return synth_fixture("small")[0]
    assert name == "c2x24"  # test_gpu_ensemble.datasets(): a partial last song block and user block
    return synth.config("c2", n_test=24).dataset()


NAMES = ("kat", "small", "c2x24")


@functools.lru_cache(maxsize=None)
def pairs(name):
    """(pair index, the stochastic draw of every pair for SEED): computed once,
    shared, never modified. The draw is reference_combination's own expression,
    hoisted out of the per-parameter call (it does not depend on the parameter)."""
    ds = dataset(name)
    idx = pair_index(ds)
    u = np.vectorize(lambda i: pair_uniform(SEED, int(i)) if i >= 0 else 2.0, otypes=[np.float64])(idx)
    idx.setflags(write=False)
    u.setflags(write=False)
    return idx, u


def restate(name, kind, ubm, ibm, param, dtype, cols=slice(None), rows=slice(None)):
    """The combination on the host, in float64 of the model dtype's values."""
    idx, u = pairs(name)
    idx, u = idx[rows, cols], u[rows, cols]
    n_pairs = dataset(name).n_pairs()
    if kind == "stochastic":  # reference_combination with the draw shared (checked against it below)
        out = np.where(u < param, ibm, ubm)
        out[idx < 0] = np.nan
    else:
        out = reference_combination(kind, ubm, ibm, param, idx, n_pairs)
    return out.astype(np.float32).astype(np.float64) if dtype == "f32" else out


def test_shared_draw_is_the_helpers_stochastic_model():
    ds = dataset("small")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        ubm, ibm = ens.model("ubm").cpu().numpy(), ens.model("ibm").cpu().numpy()
    exp = reference_combination("stochastic", ubm, ibm, 0.25, pairs("small")[0], ds.n_pairs(), seed=SEED)
    assert np.array_equal(restate("small", "stochastic", ubm, ibm, 0.25, "f64"), exp, equal_nan=True)


def materialised(ens, kind, u_t, i_t, p):
    if kind == "linear":
        return ens.linear(u_t, i_t, p)
    if kind == "aggregation":
        return ens.aggregation(u_t, i_t, p)
    return ens.stochastic(u_t, i_t, p, seed=SEED)


@pytest.mark.parametrize("n_thr", [10, 11])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sweep_map_per_value_bit_for_bit(dtype, kind, n_thr):
    for name in NAMES:
        ds = dataset(name)
        with Engine(ds, out_dtype=dtype, topk=4) as e:
            ens = DeviceEnsemble(e)
            u_t, i_t = ens.model("ubm"), ens.model("ibm")
            ubm, ibm = u_t.cpu().numpy().astype(np.float64), i_t.cpu().numpy().astype(np.float64)
            host, dev, ext = {}, {}, {}
            for p in sorted(set(PARAMS)):
                x = restate(name, kind, ubm, ibm, p, dtype)
                host[p] = evaluation.threshold_map(x, ds, THS[n_thr])
                ext[p] = (float(np.nanmin(x)), float(np.nanmax(x)))
                dev[p] = ens.threshold_map(materialised(ens, kind, u_t, i_t, p), n_thresholds=n_thr)
            if name == "small":  # the oracle itself varies over the parameters: no constant passes
                assert len(set(host.values())) >= 5, sorted(host.items())
            for P in (8, 5, 1):  # two full groups; a full and a short one; a single value
                par = PARAMS[:P]
                got = ens.sweep(kind, u_t, i_t, par, seed=SEED, n_thresholds=n_thr)
                assert len(got) == P
                for j, p in enumerate(par):
                    print(name, dtype, kind, n_thr, P, p, got[j], host[p], dev[p])
                    assert got[j] == host[p], (name, P, j, p)
                    assert got[j] == dev[p], (name, P, j, p)
                if P == 8:
                    assert got[3] == got[4]  # the two entries for 0.5
                mn, mx = e.sweep_minmax(ens_kind(kind), par, u_t.data_ptr(), i_t.data_ptr(), seed=SEED,
                                        n_pairs=ds.n_pairs())
                assert list(zip(mn.tolist(), mx.tolist())) == [ext[p] for p in par], (name, P)


def ens_kind(kind):
    from musicrecommendation_amd.ensemble import sweep_kind

    return sweep_kind(kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_class_count_block(dtype, kind):
    """The block of sweep_class_counts = the label classes' rows of the host
    counts per parameter, column for column; folded, it gives sweep_map."""
    par = PARAMS[:5]
    for name in NAMES:
        ds = dataset(name)
        for n_thr in (10, 11):
            with Engine(ds, out_dtype=dtype) as e:
                ens = DeviceEnsemble(e)
                u_t, i_t = ens.model("ubm"), ens.model("ibm")
                ubm, ibm = u_t.cpu().numpy().astype(np.float64), i_t.cpu().numpy().astype(np.float64)
                kw = dict(seed=SEED, n_pairs=ds.n_pairs())
                k = ens_kind(kind)
                mn, mx = e.sweep_minmax(k, par, u_t.data_ptr(), i_t.data_ptr(), **kw)
                cls, cpos = ens._classes()
                counts = torch.full((len(par), 2, cls.shape[0], n_thr), -7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                e.sweep_class_counts(k, par, u_t.data_ptr(), i_t.data_ptr(), mn, mx, ds.lab_off, ds.lab_songs, cls,
                                     counts.data_ptr(), n_thresholds=n_thr, **kw)
                block = counts.cpu().numpy()
                for j, p in enumerate(par):
                    x = restate(name, kind, ubm, ibm, p, dtype)
                    pred, tp = evaluation.threshold_counts(x, ds, mn[j], mx[j], THS[n_thr])
                    assert np.array_equal(block[j, 0], pred[cls]), (name, n_thr, j)
                    assert np.array_equal(block[j, 1], tp[cls]), (name, n_thr, j)
                folded = e.eval_map_counts(len(par), counts.data_ptr(), cpos, ds.n_label_songs, n_thresholds=n_thr)
                maps, mm = e.sweep_map(k, par, u_t.data_ptr(), i_t.data_ptr(), ds.lab_off, ds.lab_songs, ens.pos,
                                       ds.n_label_songs, n_thresholds=n_thr, minmax=True, **kw)
                assert folded == maps, (name, n_thr)
                assert np.array_equal(mm[:, 0], mn) and np.array_equal(mm[:, 1], mx)


def test_parameter_without_a_pair_counts_nothing():
    """Global extremes +inf / -inf (no rank holds a pair of that output): that
    parameter's block is zero, the others' are untouched by it."""
    ds = dataset("small")
    par = [0.25, 0.5, 0.75]
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        u_t, i_t = ens.model("ubm"), ens.model("ibm")
        mn, mx = e.sweep_minmax(_lib.MR_COMB_LINEAR, par, u_t.data_ptr(), i_t.data_ptr())
        cls, _cpos = ens._classes()
        blocks = []
        for lo, hi in ((mn, mx), (np.array([mn[0], np.inf, mn[2]]), np.array([mx[0], -np.inf, mx[2]]))):
            counts = torch.full((3, 2, cls.shape[0], 10), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            e.sweep_class_counts(_lib.MR_COMB_LINEAR, par, u_t.data_ptr(), i_t.data_ptr(), lo, hi, ds.lab_off,
                                 ds.lab_songs, cls, counts.data_ptr())
            blocks.append(counts.cpu().numpy())
        assert blocks[0][1].any() and not blocks[1][1].any()
        assert np.array_equal(blocks[0][[0, 2]], blocks[1][[0, 2]])


@pytest.mark.parametrize("kind", ["aggregation", "stochastic"])
def test_user_blocks_and_song_shards_sum(kind):
    """Each context alone (a block of test users with its pair_base; a song
    shard): extremes combined with min / max, class blocks added, one fold —
    the single-context sweep. The pair index, song_lo and pair_base at work."""
    ds = dataset("c2x24")
    n_pairs = ds.n_pairs()
    pos = evaluation.label_pos(ds)
    par = PARAMS[:5]
    k = ens_kind(kind)
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        u_t, i_t = ens.model("ubm"), ens.model("ibm")
        full = ens.sweep(kind, u_t, i_t, par, seed=SEED)
        full_mm = e.sweep_minmax(k, par, u_t.data_ptr(), i_t.data_ptr(), seed=SEED, n_pairs=n_pairs)
        cls, cpos = ens._classes()
    layouts = {
        "user blocks": [dict(ds=ds.subset_test_users(a, b), base=a * ds.n_songs - int(ds.te_off[a]), lo=0,
                             hi=ds.n_songs) for a, b in [(0, 7), (7, 19), (19, 24)]],
        "song shards": [dict(ds=ds, base=0, lo=lo, hi=hi) for lo, hi in song_shards(ds, 3)],
    }
    for what, parts in layouts.items():
        with contextlib.ExitStack() as stack:
            ctx = []
            for part in parts:
                e = stack.enter_context(Engine(part["ds"], out_dtype="f64", song_lo=part["lo"], song_hi=part["hi"]))
                ens = DeviceEnsemble(e, pair_base=part["base"], n_pairs=n_pairs, pos=pos,
                                     n_label_songs=ds.n_label_songs)
                u_t, i_t = ens.model("ubm"), ens.model("ibm")
                kw = dict(seed=SEED, pair_base=part["base"], n_pairs=n_pairs)
                ctx.append((e, part["ds"], u_t, i_t, kw, e.sweep_minmax(k, par, u_t.data_ptr(), i_t.data_ptr(), **kw)))
            mn = np.min([c[5][0] for c in ctx], axis=0)
            mx = np.max([c[5][1] for c in ctx], axis=0)
            assert np.array_equal(mn, full_mm[0]) and np.array_equal(mx, full_mm[1]), what
            total = np.zeros((len(par), 2, cls.shape[0], 10), dtype=np.int32)
            for e, sub, u_t, i_t, kw, _mm in ctx:
                counts = torch.empty(total.shape, dtype=torch.int32, device="cuda")
                e.sweep_class_counts(k, par, u_t.data_ptr(), i_t.data_ptr(), mn, mx, sub.lab_off, sub.lab_songs, cls,
                                     counts.data_ptr(), **kw)
                total += counts.cpu().numpy()
            up = torch.from_numpy(total).cuda()
            torch.cuda.synchronize()
            assert ctx[0][0].eval_map_counts(len(par), up.data_ptr(), cpos, ds.n_label_songs) == full, what


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_sweep_exact_at_level_boundaries(dtype):
    """The construction of test_level_thresholds_exact_at_boundaries: ubm one to
    three ulps either side of every (x - mn)/(mx - mn) = t boundary, ibm = 0.
    Linear at 1.0 is x exactly; at 0.5 it is x / 2 exactly and the extremes
    halve, so every level quotient is the same: both parameters' counts are
    eval_counts(x)'s and both mAPs are x's."""
    ds = dataset("small")
    npt = np.float32 if dtype == "f32" else np.float64
    with Engine(ds, out_dtype=dtype) as e:
        ens = DeviceEnsemble(e)
        shape = (e.n_test, e.width)
        rng = np.random.default_rng(7)
        mn, mx = npt(0.0137), npt(0.7731)
        vals = [mn, mx]
        for t in (0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9):
            x0 = npt(float(mn) + t * (float(mx) - float(mn)))
            lo = hi = x0
            for _ in range(3):
                lo, hi = np.nextafter(lo, npt(-1)), np.nextafter(hi, npt(2))
                vals += [lo, hi]
            vals.append(x0)
        x = rng.choice(np.array(vals, dtype=npt), size=shape).astype(npt)
        x[0, 0], x[0, 1] = mn, mx  # the range is exactly [mn, mx]
        heard = ds.heard_mask()[:, :e.width]
        x[heard] = np.nan
        z = np.zeros(shape, dtype=npt)
        z[heard] = np.nan
        u_t, i_t = torch.from_numpy(x).cuda(), torch.from_numpy(z).cuda()
        torch.cuda.synchronize()
        par = [1.0, 0.5]
        kw = dict(n_pairs=ds.n_pairs())
        got_mn, got_mx = e.sweep_minmax(_lib.MR_COMB_LINEAR, par, u_t.data_ptr(), i_t.data_ptr(), **kw)
        xmn, xmx = float(np.nanmin(x)), float(np.nanmax(x))
        assert got_mn.tolist() == [xmn, xmn / 2] and got_mx.tolist() == [xmx, xmx / 2]
        pred, tp = e.eval_counts(u_t.data_ptr(), xmn, xmx, ds.lab_off, ds.lab_songs)
        cls, _cpos = ens._classes()
        counts = torch.empty((2, 2, cls.shape[0], 10), dtype=torch.int32, device="cuda")
        e.sweep_class_counts(_lib.MR_COMB_LINEAR, par, u_t.data_ptr(), i_t.data_ptr(), got_mn, got_mx, ds.lab_off,
                             ds.lab_songs, cls, counts.data_ptr(), **kw)
        block = counts.cpu().numpy()
        for j in range(2):
            assert np.array_equal(block[j, 0], pred[cls]), j
            assert np.array_equal(block[j, 1], tp[cls]), j
        exp = evaluation.threshold_map(x.astype(np.float64), ds)
        assert ens.sweep("linear", u_t, i_t, par) == [exp, exp]


@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_range(kind):
    """ubm = ibm = one constant: min == max for every parameter, nothing passes
    a level; the mAP is the materialised path's, the same for every parameter."""
    ds = dataset("small")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        c = np.full((e.n_test, e.width), 0.375)
        c[ds.heard_mask()[:, :e.width]] = np.nan
        u_t = torch.from_numpy(c).cuda()
        i_t = u_t.clone()
        torch.cuda.synchronize()
        par = PARAMS[:5]
        mn, mx = e.sweep_minmax(ens_kind(kind), par, u_t.data_ptr(), i_t.data_ptr(), seed=SEED, n_pairs=ds.n_pairs())
        assert np.array_equal(mn, mx)
        got = ens.sweep(kind, u_t, i_t, par, seed=SEED)
        exp = [ens.threshold_map(materialised(ens, kind, u_t, i_t, p)) for p in par]
        assert got == exp and len(set(got)) == 1


def test_errors():
    ds = dataset("small")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        u_t, i_t = ens.model("ubm"), ens.model("ibm")
        with pytest.raises(_lib.EngineError):
            ens.aggregation(u_t, i_t, 1.2)  # as today
        with pytest.raises(_lib.EngineError):
            ens.sweep("aggregation", u_t, i_t, [0.5, 1.2])
        with pytest.raises(_lib.EngineError):
            ens.sweep("stochastic", u_t, i_t, [-0.1])
        with pytest.raises(_lib.EngineError):
            ens.sweep("linear", u_t, i_t, [])
        with pytest.raises(_lib.EngineError):
            ens.sweep("linear", u_t, i_t, [i / 64 for i in range(65)])
        assert len(ens.sweep("linear", u_t, i_t, [i / 63 for i in range(64)])) == 64  # the cap itself is legal
        with pytest.raises(_lib.EngineError):
            ens.sweep(7, u_t, i_t, [0.5])
        with pytest.raises(_lib.EngineError):
            ens.sweep("linear", u_t, i_t, [0.5], n_thresholds=9)
        with pytest.raises(_lib.EngineError):
            e.sweep_minmax(_lib.MR_COMB_AGGREGATION, [0.5], u_t.data_ptr(), i_t.data_ptr(), pair_base=-1)
        assert ens.sweep("linear", u_t, i_t, [1.7]) == [ens.threshold_map(ens.linear(u_t, i_t, 1.7))]  # linear: any alpha


def test_driver_and_mirror(tmp_path, capsys):
    ds, z = synth_fixture("small")
    n, m = 60, 8
    paths = []
    for kind, key in (("train", "train"), ("test", "test"), ("test_labels", "labels")):
        p = tmp_path / f"{kind}_{n}_{m}.txt"
        p.write_text("".join(l + "\n" for l in z[key].tolist()))
        paths.append(os.fspath(p))
    grid = [0.0, 0.25, 0.5, 0.75, 1.0]
    plain = driver.run(n, m, os.fspath(tmp_path), verbose=False)
    capsys.readouterr()
    swept = driver.run(n, m, os.fspath(tmp_path), verbose=False, sweeps=["linear:0:1:5"])
    out = capsys.readouterr().out
    assert "sweeps" not in plain and swept["mAP"] == plain["mAP"]
    assert {k: v for k, v in swept.items() if k != "sweeps"} == plain
    with Engine(ds, out_dtype="f64", topk=10) as e:
        ens = DeviceEnsemble(e)
        exp = ens.sweep("linear", ens.model("ubm"), ens.model("ibm"), grid)
    (s,) = swept["sweeps"]
    assert s["kind"] == "linear" and s["params"] == grid and s["mAP"] == exp
    assert s["best"] == grid[int(np.argmax(exp))]
    lines = [l for l in out.splitlines() if l.startswith("linear sweep ")]
    assert lines[:5] == [f"linear sweep {p} mAP: {driver.round_at(10, v)}" for p, v in zip(grid, exp)]
    assert len(lines) == 6 and lines[5].startswith(f"linear sweep best: {s['best']} mAP: ")
    dist = driver.run(n, m, os.fspath(tmp_path), verbose=False, distributed=True, seed=5,
                      sweeps=["stochastic:0.25:0.75:3"])
    with Engine(ds, out_dtype="f64", topk=10) as e:
        ens = DeviceEnsemble(e)
        assert dist["sweeps"][0]["mAP"] == ens.sweep("stochastic", ens.model("ubm"), ens.model("ibm"),
                                                     [0.25, 0.5, 0.75], seed=5, n_thresholds=11)
    mr = MusicRecommender(*paths)
    try:
        assert mr.sweepCombinationModel("linear", grid) == list(zip(grid, exp))
    finally:
        mr.close()
