"""The asymmetric-cosine, locality-q item-based model on the device
(csrc/mr_asym.hip): mr_ibm_asym_device against its numpy twin
evaluation.asym_item_model, bit for bit (f32 contexts: against the twin rounded
once) — on the fixtures, across song tiles, song sub-ranges and song shards, in
every launch shape, on a hand-built dataset whose counts pass 4,096; its
identities at (0.5, 1) against the similar-song rows and the engine's own
ItemBasedModel; the ranking, mAP and combinations downstream; the argument
checks; the front ends."""
import ctypes
import os

import numpy as np
import pytest

from musicrecommendation_amd import _lib, driver, evaluation, synth
from musicrecommendation_amd.engine import Engine, rank_map_host
from musicrecommendation_amd.ensemble import DeviceEnsemble
from musicrecommendation_amd.recommender import MusicRecommender

from helpers import GOLDEN, dataset_from_lines, kat, synth_fixture

pytestmark = pytest.mark.gpu

GRID = [(0.5, 1), (0.15, 3), (0.0, 1), (1.0, 2), (0.85, 8)]
_ds = {}
_twin = {}


def dataset(name):
    if name not in _ds:
        if name == "kat":
            K = kat()
            _ds[name] = dataset_from_lines(K["train"], K["test"], K["labels"])
        elif name == "small":
            _ds[name] = synth_fixture("small")[0]
        elif name == "hand":
            _ds[name] = hand_dataset()
        else:
            _ds[name] = synth.config(name).dataset()
    return _ds[name]


def twin(name, alpha, q):
    """The twin's full model, computed once per (dataset, alpha, q) and never written to."""
    key = (name, alpha, q)
    if key not in _twin:
        t = evaluation.asym_item_model(dataset(name), alpha, q)
        t.setflags(write=False)
        _twin[key] = t
    return _twin[key]


def check_model(t, exp, dtype="f64"):
    """NaN in the same places, every other value bit-equal (f32: to the twin rounded once)."""
    got = t.cpu().numpy()
    if dtype == "f32":
        exp = exp.astype(np.float32)
        assert got.dtype == np.float32
        view = np.int32
    else:
        assert got.dtype == np.float64
        view = np.int64
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(got[ok].view(view), exp[ok].view(view))
    return got


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["kat", "small"])
def test_fixtures_bitwise_against_the_twin(name, dtype):
    ds = dataset(name)
    with Engine(ds, out_dtype=dtype) as e:
        ens = DeviceEnsemble(e)
        for alpha, q in GRID:
            exp = twin(name, alpha, q)
            got = check_model(ens.item_based(alpha, q), exp, dtype)
            assert np.array_equal(np.isnan(got), ds.heard_mask())  # the NaN pattern is T(u)
            assert np.count_nonzero(np.nan_to_num(exp)) > 0
        check_model(ens.item_based(), twin(name, 0.5, 1), dtype)  # the defaults are the reference's model


def test_tiles_sub_ranges_and_song_shards(monkeypatch):
    """synth_small in tiles of 256 songs (9 tiles, the last one partial): plain;
    with the sub-range lowered to 100 songs (passes of 100, 100 and 56 per
    tile); and as three unaligned song shards, concatenated by column."""
    ds = dataset("small")
    n = ds.n_songs
    for alpha, q in ((0.15, 3), (0.5, 1)):
        exp = twin("small", alpha, q)
        with Engine(ds, block_songs=256, stage1="separate", out_dtype="f64") as e:
            assert e.block_songs == 256 and e.n_tiles == (n + 255) // 256 == 9 and n % 256 != 0
            one = check_model(DeviceEnsemble(e).item_based(alpha, q), exp)
            monkeypatch.setenv("MR_ASYM_SUB", "100")
            check_model(DeviceEnsemble(e).item_based(alpha, q), exp)
            monkeypatch.delenv("MR_ASYM_SUB")
        parts = []
        for lo, hi in ((0, 333), (333, 900), (900, n)):  # not tile-aligned
            with Engine(ds, block_songs=256, stage1="separate", out_dtype="f64", song_lo=lo, song_hi=hi) as e:
                assert e.n_tiles > 1 and (e.song_lo, e.song_hi) == (lo, hi)
                parts.append(check_model(DeviceEnsemble(e).item_based(alpha, q), exp[:, lo:hi]))
        cat = np.concatenate(parts, axis=1)
        assert np.array_equal(cat.view(np.int64), one.view(np.int64))  # NaN payloads included


def test_every_launch_shape_gives_identical_bits():
    ds = dataset("small")
    exp = twin("small", 0.15, 3)
    shapes = [("fused", dict(stage1="fused")),
              ("separate", dict(stage1="separate", topk=64)),
              ("wide", dict(stage1="wide", ibm_route="two_hop")),
              ("wide", dict(stage1="wide", ibm_route="cooc")),
              ("wide", dict(stage1="wide", train_order="given")),
              (None, dict(train_order="given"))]
    first = None
    for shape, kw in shapes:
        with Engine(ds, out_dtype="f64", **kw) as e:
            assert shape is None or e.shape == shape
            if "ibm_route" in kw:
                assert e.ibm_route == kw["ibm_route"]
            got = check_model(DeviceEnsemble(e).item_based(0.15, 3), exp)
        if first is None:
            first = got
        else:
            assert np.array_equal(got.view(np.int64), first.view(np.int64))


N_HAND = 5000


def hand_dataset():
    """5,000 train users who all heard A and B plus one song of their own out of
    600 (S000..S599, user v hears S(v mod 600): 9 listeners for the first 200, 8
    for the others). Test users: x0 heard A and the test-only song TEST; x1
    heard only TEST and TEST2, songs without a train listener; x2 heard S000
    to S299."""
    train = []
    for v in range(N_HAND):
        train += [f"u{v:05d}\tA\t1", f"u{v:05d}\tB\t1", f"u{v:05d}\tS{v % 600:03d}\t1"]
    test = ["x0\tTEST\t1", "x0\tA\t1", "x1\tTEST\t1", "x1\tTEST2\t1"] + [f"x2\tS{i:03d}\t1" for i in range(300)]
    ds = dataset_from_lines(train, test, ["x0\tB\t1", "x2\tA\t1"])
    assert (ds.n_train, ds.n_test, ds.n_songs) == (N_HAND, 3, 604)
    return ds


@pytest.mark.parametrize("alpha,q", [(0.5, 1), (0.15, 3), (1.0, 2)])
def test_hand_built_heavy_counters_long_lists_and_ties(alpha, q):
    ds = dataset("hand")
    si = {ds.song_names(i): i for i in range(ds.n_songs)}
    ui = {ds.test_names(i): i for i in range(ds.n_test)}
    exp = twin("hand", alpha, q)
    pa, pb = evaluation.asym_tables(alpha, ds.song_count)
    # the twin's own numbers, by hand: x0 has one heard song with listeners, A (c(A) has x0's line)
    w = N_HAND / (pa[si["B"]] * pb[si["A"]])
    t = w
    for _ in range(q - 1):
        t = t * w
    assert exp[ui["x0"], si["B"]] == t and t > 0
    a, b = si["S300"], si["S301"]
    assert exp[ui["x0"], a].view(np.int64) == exp[ui["x0"], b].view(np.int64) != 0  # a pair of bit-equal scores
    assert int(ds.te_off[ui["x2"] + 1] - ds.te_off[ui["x2"]]) == 300
    with Engine(ds, out_dtype="f64") as e:
        assert e.shape == "wide"  # chosen automatically at 5,000 train users
        got = check_model(DeviceEnsemble(e).item_based(alpha, q), exp)
    assert got[ui["x0"], a].view(np.int64) == got[ui["x0"], b].view(np.int64)
    lonely = got[ui["x1"]]
    heard = ds.heard_mask()[ui["x1"]]
    assert heard.sum() == 2 and np.isnan(lonely[heard]).all()
    assert (lonely[~heard].view(np.int64) == 0).all()  # all +0.0, never NaN, never -0.0
    assert np.count_nonzero(np.nan_to_num(got[ui["x2"]])) >= 2  # A and B against 300 heard songs


def test_identities_at_half_one_on_c1():
    """At (0.5, 1), all users of C1: the model is the NumPy left fold,
    ascending s2, of the dense rows similar_songs returns for T(u), bit for bit
    (the denominator is the same product with its factors swapped), and within
    the project's literal-versus-fixed-point bound, 1e-7 relative, of the
    engine's own ItemBasedModel wherever that is non-zero; zeros coincide."""
    ds = dataset("c1")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        got = ens.item_based(0.5, 1).cpu().numpy()
        ibm = e.score_dense("ibm")
        fold = np.empty_like(got)
        for u in range(ds.n_test):
            mine = np.sort(np.asarray(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]]))
            rows = ens.similar_songs(mine, 0, dense=True)[2].cpu().numpy()
            acc = np.zeros(ds.n_songs)
            for r in rows:                       # ascending s2
                acc = acc + np.nan_to_num(r)     # a row's own NaN (s == s2) is a heard column
            acc[mine] = np.nan
            fold[u] = acc
    assert np.array_equal(np.isnan(got), ds.heard_mask()) and np.array_equal(np.isnan(fold), np.isnan(got))
    ok = ~np.isnan(got)
    assert np.array_equal(got[ok].view(np.int64), fold[ok].view(np.int64))
    assert np.array_equal(np.isnan(ibm), np.isnan(got))
    a, b = got[ok], ibm[ok]
    assert np.array_equal(a == 0, b == 0) and np.count_nonzero(b) > 0  # a zero in one is a zero in the other
    nz = b != 0
    rel = np.abs(a[nz] - b[nz]) / np.abs(b[nz])
    print(f"asym(0.5, 1) against ibm on C1: max relative error {rel.max():.3e} over {nz.sum()} non-zero pairs")
    assert (rel <= 1e-7).all()


def test_downstream_rank_map_and_combination():
    ds = dataset("small")
    exp = twin("small", 0.15, 3)
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        model = ens.item_based(0.15, 3)
        for K in (10, 1024):
            songs, scores = ens.rank(model, K)
            e_songs, e_scores = evaluation.rank_lists(exp, K)
            songs, scores = songs.cpu().numpy(), scores.cpu().numpy()
            assert np.array_equal(songs, e_songs)
            full = e_songs >= 0
            assert np.array_equal(scores[full].view(np.int64), e_scores[full].view(np.int64))
            assert np.isnan(scores[~full]).all()
        # mAP@10: mr_rank_map_host over the twin's lists is the CPU value, in the same summation
        # order (bit-equal); evaluation.map_at_k sums in another order (the project's 1e-12)
        cpu = rank_map_host(evaluation.rank_lists(exp, 10)[0], 10, ds.lab_off, ds.lab_songs)[0]
        dev = ens.map_at(model, 10)
        assert np.float64(dev).view(np.int64) == np.float64(cpu).view(np.int64)
        assert abs(dev - evaluation.map_at_k(evaluation.rank_lists(exp, 10)[0], ds, k=10)) <= 1e-12
        ubm = ens.model("ubm")
        lin = ens.linear(ubm, model, 0.5).cpu().numpy()
        want = ubm.cpu().numpy() * 0.5 + exp * (1 - 0.5)  # MR:317-351's expression
        assert np.array_equal(np.isnan(lin), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(lin[ok].view(np.int64), want[ok].view(np.int64))
        assert ens.threshold_map(model) == evaluation.threshold_map(exp, ds)


def test_errors_leave_the_output_untouched():
    import torch

    ds = dataset("kat")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        out = torch.full((e.n_test, e.width), 2.5, dtype=torch.float64, device=ens.device)
        for alpha in (-0.1, 1.1, float("nan")):
            with pytest.raises(_lib.EngineError) as ei:
                e.ibm_asym(alpha, 1, out.data_ptr())
            assert ei.value.code == _lib.MR_E_INVALID
            torch.cuda.synchronize()
            assert (out == 2.5).all()
        for q in (0, 9):
            with pytest.raises(_lib.EngineError) as ei:
                e.ibm_asym(0.5, q, out.data_ptr())
            assert ei.value.code == _lib.MR_E_INVALID
            torch.cuda.synchronize()
            assert (out == 2.5).all()
        with pytest.raises(_lib.EngineError) as ei:
            e.ibm_asym(0.5, 1, 0)  # NULL dense_dev
        assert ei.value.code == _lib.MR_E_INVALID
        # a context that was created but never loaded: MR_E_STATE, nothing written
        L = _lib.lib()
        opt = _lib.MrOptions()
        assert L.mr_options_default(ctypes.byref(opt)) == _lib.MR_OK
        h = ctypes.c_void_p()
        assert L.mr_create(ctypes.byref(opt), ctypes.byref(h)) == _lib.MR_OK
        try:
            assert L.mr_ibm_asym_device(h, 0.5, 1, ctypes.c_void_p(out.data_ptr())) == _lib.MR_E_STATE
            assert L.mr_ibm_asym_device(h, 0.5, 0, ctypes.c_void_p(out.data_ptr())) == _lib.MR_E_INVALID  # q before state
        finally:
            L.mr_destroy(h)
        torch.cuda.synchronize()
        assert (out == 2.5).all()
        e.ibm_asym(0.5, 1, out.data_ptr())  # and the same buffer is filled by a good call
        check_model(out, twin("kat", 0.5, 1))


def test_recommender_front_ends():
    K = kat()
    ds = dataset("kat")
    rec = MusicRecommender(K["train"], K["test"], K["labels"])
    try:
        for alpha, q in ((0.15, 3), (0.5, 1)):
            model = rec.getAsymmetricItemBasedModel(alpha, q)
            want = rec._to_model(np.array(twin("kat", alpha, q)))  # getItemBasedModel's shape and order
            assert len(model) == ds.n_pairs() == len(want)
            assert [(u, s) for u, (s, _x) in model] == [(u, s) for u, (s, _x) in want]
            assert [x for _u, (_s, x) in model] == [x for _u, (_s, x) in want]  # exact
        assert [(u, s) for u, (s, _x) in model] == [(u, s) for u, (s, _x) in rec.getItemBasedModel()]
        alphas, qs = (0.15, 0.5), (1, 3)
        got = rec.sweepItemSimilarity(alphas, qs, k=10)
        assert [(a, q) for a, q, _m in got] == [(0.15, 1), (0.15, 3), (0.5, 1), (0.5, 3)]
        for a, q, m in got:
            lists = evaluation.rank_lists(twin("kat", a, q), 10)[0]
            print(f"alpha {a} q {q}: device mAP@10 {m!r} numpy {evaluation.map_at_k(lists, ds, k=10)!r}")
            # the same lists; the two folds differ in summation order only (at most n_test * k terms
            # of at most 1 each, far inside the project's 1e-12 for this bound)
            assert abs(m - evaluation.map_at_k(lists, ds, k=10)) <= 1e-12
            assert np.float64(m).view(np.int64) == np.float64(rank_map_host(lists, 10, ds.lab_off, ds.lab_songs)[0]).view(np.int64)
    finally:
        rec.close()


def test_driver_asym(tmp_path, capsys):
    z = np.load(os.path.join(GOLDEN, "synth_small.npz"))
    n_tr = len({l.split("\t")[0] for l in z["train"].tolist()})
    n_te = len({l.split("\t")[0] for l in z["test"].tolist()})
    for key, fn in (("train", "train"), ("test", "test"), ("labels", "test_labels")):
        (tmp_path / f"{fn}_{n_tr}_{n_te}.txt").write_text("".join(l + "\n" for l in z[key].tolist()))
    out = driver.run(n_tr, n_te, str(tmp_path), asym=(0.15, 3), recommend=10)
    ds = dataset("small")
    exp = twin("small", 0.15, 3)
    name = "asymmetricItemBasedModel"
    assert out["asym"] == {"alpha": 0.15, "q": 3}
    assert list(out["mAP"])[-1] == name and len(out["mAP"]) == 6
    assert out["mAP"][name] == evaluation.threshold_map(exp, ds)
    lists = evaluation.rank_lists(exp, 10)[0]
    assert np.float64(out["mAP@K"][name]).view(np.int64) == \
        np.float64(rank_map_host(lists, 10, ds.lab_off, ds.lab_songs)[0]).view(np.int64)
    text = capsys.readouterr().out
    assert f"Elapsed time for {name} (alpha 0.15, q 3):\t" in text
    assert f"Elapsed time for {name} model mAP:\t" in text
    assert f"{name} model mAP: {driver.round_at(10, out['mAP'][name])}" in text
    assert f"{name} model mAP@10: {driver.round_at(10, out['mAP@K'][name])}" in text
