"""The asymmetric-cosine, locality-q user-based model on the device
(csrc/mr_uasym.hip): mr_ubm_asym_device against its numpy twin
evaluation.asym_user_model, bit for bit (f32 contexts: against the twin rounded
once) — on the fixtures at three fraction-bit counts, through the later
iterations of every host loop (train-user chunks, test-user batches, song
sub-ranges, launch rows, song shards), in every launch shape, on a hand-built
dataset of 5,000 train users; its identity with the engine's own UserBasedModel
at (0.5, 1); the headroom rule and the argument checks; the ranking, mAP and
combinations downstream; the front ends. No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from musicrecommendation_amd import _lib, driver, evaluation, synth
from musicrecommendation_amd.engine import Engine, rank_map_host
from musicrecommendation_amd.ensemble import DeviceEnsemble
from musicrecommendation_amd.recommender import MusicRecommender

from helpers import dataset_from_lines, kat, synth_fixture

pytestmark = pytest.mark.gpu

GRID = [(0.5, 1), (0.15, 3), (0.0, 1), (1.0, 2), (0.85, 8)]
ENV = ("MR_UASYM_CHUNK", "MR_UASYM_BATCH", "MR_UASYM_SUB", "MR_LAUNCH_ROWS")
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


def twin(name, alpha, q, F=32):
    """The twin's full model, computed once per (dataset, alpha, q, F) and never written to."""
    key = (name, alpha, q, F)
    if key not in _twin:
        t = evaluation.asym_user_model(dataset(name), alpha, q, F)
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


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["kat", "small"])
def test_fixtures_bitwise_against_the_twin(name, dtype):
    ds = dataset(name)
    with Engine(ds, out_dtype=dtype) as e:
        ens = DeviceEnsemble(e)
        for alpha, q in GRID:
            for arg, F in ((None, 32), (40, 40), (52, 52)):  # None: the context's frac_bits
                exp = twin(name, alpha, q, F)
                got = check_model(ens.user_based(alpha, q, arg), exp, dtype)
                assert np.array_equal(np.isnan(got), ds.heard_mask())  # the NaN pattern is T(u)
                assert np.count_nonzero(np.nan_to_num(exp)) > 0


@pytest.mark.parametrize("name", ["kat", "small", "c1"])
def test_the_defaults_are_the_engines_user_based_model(name):
    ds = dataset(name)
    for F in (32, 24):  # the call's frac_bits left at 0: the context's
        with Engine(ds, out_dtype="f64", frac_bits=F) as e:
            ens = DeviceEnsemble(e)
            ubm = ens.model("ubm").cpu().numpy()
            got = check_model(ens.user_based(), ubm)
            assert np.array_equal(np.isnan(got), ds.heard_mask()) and np.count_nonzero(np.nan_to_num(got)) > 0
            if name != "c1":
                check_model(ens.user_based(), twin(name, 0.5, 1, F))


def test_every_loop_reaches_its_later_iterations(monkeypatch):
    """synth_small (60 train, 8 test users, 2,273 songs) in tiles of 256 songs (9
    tiles, the last one partial) at (0.15, 3): plain; 4 train-user chunks, the
    last one partial; batches of 3, 3 and 2 test users; sub-ranges of 100, 100
    and 56 songs per tile; 8 rows per launch; all of these at once; and as
    three unaligned song shards, concatenated by column."""
    ds = dataset("small")
    n = ds.n_songs
    assert (ds.n_train, ds.n_test) == (60, 8)
    alpha, q = 0.15, 3
    exp = twin("small", alpha, q)
    settings = [{}, {"MR_UASYM_CHUNK": "16"}, {"MR_UASYM_BATCH": "3"}, {"MR_UASYM_SUB": "100"},
                {"MR_LAUNCH_ROWS": "8"},
                {"MR_UASYM_CHUNK": "16", "MR_UASYM_BATCH": "3", "MR_UASYM_SUB": "100", "MR_LAUNCH_ROWS": "8"}]
    runs = []
    with Engine(ds, block_songs=256, stage1="separate", out_dtype="f64") as e:
        assert e.block_songs == 256 and e.n_tiles == (n + 255) // 256 == 9 and n % 256 != 0
        for env in settings:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            runs.append(check_model(DeviceEnsemble(e).user_based(alpha, q), exp))
            for k in env:
                monkeypatch.delenv(k)
    for env in (settings[0], settings[-1]):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        parts = []
        for lo, hi in ((0, 333), (333, 900), (900, n)):  # not tile-aligned
            with Engine(ds, block_songs=256, stage1="separate", out_dtype="f64", song_lo=lo, song_hi=hi) as e:
                assert e.n_tiles > 1 and (e.song_lo, e.song_hi) == (lo, hi)
                parts.append(check_model(DeviceEnsemble(e).user_based(alpha, q), exp[:, lo:hi]))
        runs.append(np.concatenate(parts, axis=1))
    for r in runs[1:]:
        assert np.array_equal(r.view(np.int64), runs[0].view(np.int64))  # NaN payloads included


def test_launch_rows_split_a_batch_on_c1(monkeypatch):
    """C1 has 10 test users, two more than the smallest MR_LAUNCH_ROWS: launches
    of 8 and 2 rows per kernel, and with batches of 9 users rows 8 + 1, then 1."""
    ds = dataset("c1")
    assert ds.n_test == 10
    exp = twin("c1", 0.15, 3)
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        plain = check_model(ens.user_based(0.15, 3), exp)
        monkeypatch.setenv("MR_LAUNCH_ROWS", "8")
        rows = check_model(ens.user_based(0.15, 3), exp)
        monkeypatch.setenv("MR_UASYM_BATCH", "9")
        both = check_model(ens.user_based(0.15, 3), exp)
    assert np.array_equal(rows.view(np.int64), plain.view(np.int64))
    assert np.array_equal(both.view(np.int64), plain.view(np.int64))


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
            got = check_model(DeviceEnsemble(e).user_based(0.15, 3), exp)
        if first is None:
            first = got
        else:
            assert np.array_equal(got.view(np.int64), first.view(np.int64))


N_HAND = 5000


def hand_dataset():
    """5,000 train users who all heard A plus one song of their own out of 600
    (S000..S599, user v hears S(v mod 600)). Train user u00000 also heard
    W000..W299 (300 consecutive song ids); u00001's line for A is there twice
    (tr_len 3, two distinct songs). Test users: x0 heard A and the test-only
    song TEST; x1 heard only TEST and TEST2, songs without a train listener; x2
    heard S000 to S299; x3 and x4 both heard A and S005."""
    train = []
    for v in range(N_HAND):
        train += [f"u{v:05d}\tA\t1", f"u{v:05d}\tS{v % 600:03d}\t1"]
    train += [f"u00000\tW{i:03d}\t1" for i in range(300)]
    train += ["u00001\tA\t1"]
    test = ["x0\tTEST\t1", "x0\tA\t1", "x1\tTEST\t1", "x1\tTEST2\t1"] + [f"x2\tS{i:03d}\t1" for i in range(300)]
    test += ["x3\tA\t1", "x3\tS005\t1", "x4\tA\t1", "x4\tS005\t1"]
    ds = dataset_from_lines(train, test, ["x0\tS001\t1", "x2\tA\t1"])
    assert (ds.n_train, ds.n_test, ds.n_songs) == (N_HAND, 5, 903)
    return ds


@pytest.mark.parametrize("alpha,q", [(0.5, 1), (0.15, 3), (1.0, 2)])
def test_hand_built_long_lists_long_rows_and_equal_users(alpha, q, monkeypatch):
    ds = dataset("hand")
    si = {ds.song_names(i): i for i in range(ds.n_songs)}
    ui = {ds.test_names(i): i for i in range(ds.n_test)}
    vi = {ds.train_names(i): i for i in range(ds.n_train)}
    deg, tr_len = np.diff(ds.tr_off), np.asarray(ds.tr_len)
    assert deg[vi["u00000"]] == 302 and si["W299"] - si["W000"] == 299
    assert tr_len[vi["u00001"]] == 3 > deg[vi["u00001"]] == 2
    assert int(ds.te_off[ui["x2"] + 1] - ds.te_off[ui["x2"]]) == 300
    assert ds.te_len[ui["x3"]] == ds.te_len[ui["x4"]]
    exp = twin("hand", alpha, q)
    # the twin's own numbers, by hand: x3's neighbour u00001 heard A only among x3's songs
    pa = evaluation.asym_tables(alpha, ds.te_len)[0]
    pb = evaluation.asym_tables(alpha, ds.tr_len)[1]
    w = 1.0 / (pa[ui["x3"]] * pb[vi["u00001"]])
    t = w
    for _ in range(q - 1):
        t = t * w
    nb, keys = evaluation.asym_user_keys(ds, alpha, q, 32, users=[ui["x3"]])[0]
    assert nb.size == N_HAND and keys[nb == vi["u00001"]][0] == int(np.rint(t * 2.0 ** 32)) > 0
    monkeypatch.setenv("MR_UASYM_CHUNK", "2048")  # 3 chunks, the last one partial
    with Engine(ds, out_dtype="f64") as e:
        assert e.shape == "wide"  # chosen automatically at 5,000 train users
        assert si["W000"] // e.block_songs == si["W299"] // e.block_songs  # u00000's 300 songs lie in one tile
        got = check_model(DeviceEnsemble(e).user_based(alpha, q), exp)
    assert np.array_equal(got[ui["x3"]].view(np.int64), got[ui["x4"]].view(np.int64))
    lonely = got[ui["x1"]]
    heard = ds.heard_mask()[ui["x1"]]
    assert heard.sum() == 2 and np.isnan(lonely[heard]).all()
    assert (lonely[~heard].view(np.int64) == 0).all()  # all +0.0, never NaN, never -0.0
    assert got[ui["x0"], si["W000"]] > 0 and got[ui["x2"], si["A"]] > 0


def test_headroom_rule_on_the_hand_built_dataset(monkeypatch):
    """max c_tr = 5,000 needs 13 bits: frac_bits 49 is the last one allowed."""
    import torch

    ds = dataset("hand")
    monkeypatch.setenv("MR_UASYM_CHUNK", "2048")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        check_model(ens.user_based(0.15, 3, 49), twin("hand", 0.15, 3, 49))
        out = torch.full((e.n_test, e.width), 2.5, dtype=torch.float64, device=ens.device)
        torch.cuda.synchronize()
        for F in (50, 52):
            with pytest.raises(_lib.EngineError) as ei:
                e.ubm_asym(0.15, 3, out.data_ptr(), F)
            assert ei.value.code == _lib.MR_E_INVALID
        torch.cuda.synchronize()
        assert (out == 2.5).all()


def test_errors_leave_the_output_untouched():
    import torch

    ds = dataset("kat")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        out = torch.full((e.n_test, e.width), 2.5, dtype=torch.float64, device=ens.device)
        torch.cuda.synchronize()
        bad = [dict(alpha=a) for a in (-0.1, 1.1, float("nan"))] + [dict(q=q) for q in (0, 9)] + \
              [dict(frac_bits=F) for F in (-1, 7, 53)]
        for kw in bad:
            args = dict(alpha=0.5, q=1, frac_bits=0)
            args.update(kw)
            with pytest.raises(_lib.EngineError) as ei:
                e.ubm_asym(args["alpha"], args["q"], out.data_ptr(), args["frac_bits"])
            assert ei.value.code == _lib.MR_E_INVALID
            torch.cuda.synchronize()
            assert (out == 2.5).all()
        with pytest.raises(_lib.EngineError) as ei:
            e.ubm_asym(0.5, 1, 0)  # NULL dense_dev
        assert ei.value.code == _lib.MR_E_INVALID
        # a context that was created but never loaded: MR_E_STATE, nothing written
        L = _lib.lib()
        opt = _lib.MrOptions()
        assert L.mr_options_default(ctypes.byref(opt)) == _lib.MR_OK
        h = ctypes.c_void_p()
        assert L.mr_create(ctypes.byref(opt), ctypes.byref(h)) == _lib.MR_OK
        try:
            ptr = ctypes.c_void_p(out.data_ptr())
            assert L.mr_ubm_asym_device(h, 0.5, 1, 0, ptr) == _lib.MR_E_STATE
            assert L.mr_ubm_asym_device(h, 0.5, 0, 0, ptr) == _lib.MR_E_INVALID  # q before state
            assert L.mr_ubm_asym_device(h, 0.5, 1, 53, ptr) == _lib.MR_E_INVALID  # frac_bits before state
        finally:
            L.mr_destroy(h)
        torch.cuda.synchronize()
        assert (out == 2.5).all()
        e.ubm_asym(0.5, 1, out.data_ptr())  # and the same buffer is filled by a good call
        check_model(out, twin("kat", 0.5, 1))


def test_downstream_rank_map_and_combination():
    ds = dataset("small")
    exp = twin("small", 0.15, 3)
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        model = ens.user_based(0.15, 3)
        songs, scores = ens.rank(model, 10)
        e_songs, e_scores = evaluation.rank_lists(exp, 10)
        songs, scores = songs.cpu().numpy(), scores.cpu().numpy()
        assert np.array_equal(songs, e_songs)
        full = e_songs >= 0
        assert np.array_equal(scores[full].view(np.int64), e_scores[full].view(np.int64))
        assert np.isnan(scores[~full]).all()
        # mAP@10: mr_rank_map_host over the twin's lists is the CPU value in the device's summation order
        cpu = rank_map_host(e_songs, 10, ds.lab_off, ds.lab_songs)[0]
        dev = ens.map_at(model, 10)
        assert np.float64(dev).view(np.int64) == np.float64(cpu).view(np.int64)
        item = evaluation.asym_item_model(ds, 0.15, 3)
        lin = ens.linear(model, ens.item_based(0.15, 3), 0.5).cpu().numpy()
        want = exp * 0.5 + item * (1 - 0.5)  # MR:317-351's expression
        assert np.array_equal(np.isnan(lin), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(lin[ok].view(np.int64), want[ok].view(np.int64))
        assert ens.threshold_map(model) == evaluation.threshold_map(exp, ds)


def test_recommender_front_ends():
    K = kat()
    ds = dataset("kat")
    rec = MusicRecommender(K["train"], K["test"], K["labels"])
    try:
        for alpha, q, F in ((0.15, 3, None), (0.5, 1, None), (0.85, 8, 52)):
            model = rec.getAsymmetricUserBasedModel(alpha, q, F)
            want = rec._to_model(np.array(twin("kat", alpha, q, F or 32)))  # getUserBasedModel's shape and order
            assert len(model) == ds.n_pairs() == len(want)
            assert [(u, s) for u, (s, _x) in model] == [(u, s) for u, (s, _x) in want]
            assert [x for _u, (_s, x) in model] == [x for _u, (_s, x) in want]  # exact
        assert rec.getAsymmetricUserBasedModel(0.5, 1) == rec.getUserBasedModel()
        alphas, qs = (0.15, 0.5), (1, 3)
        got = rec.sweepUserSimilarity(alphas, qs, k=10)
        assert [(a, q) for a, q, _m in got] == [(0.15, 1), (0.15, 3), (0.5, 1), (0.5, 3)]
        ens = DeviceEnsemble(rec.engine())
        for a, q, m in got:
            lists = evaluation.rank_lists(twin("kat", a, q), 10)[0]
            print(f"alpha {a} q {q}: device mAP@10 {m!r}")
            assert m == ens.map_at(ens.user_based(a, q), 10)
            assert np.float64(m).view(np.int64) == \
                np.float64(rank_map_host(lists, 10, ds.lab_off, ds.lab_songs)[0]).view(np.int64)
        assert rec.sweepUserSimilarity((0.85,), (8,), k=10, frac_bits=52)[0][2] == \
            ens.map_at(ens.user_based(0.85, 8, 52), 10)
    finally:
        rec.close()


def test_driver_asym_user(tmp_path, capsys):
    K = kat()
    ds = dataset("kat")
    for key, fn in (("train", "train"), ("test", "test"), ("labels", "test_labels")):
        (tmp_path / f"{fn}_{ds.n_train}_{ds.n_test}.txt").write_text("".join(l + "\n" for l in K[key]))
    out = driver.run(ds.n_train, ds.n_test, str(tmp_path), asym_user="0.3:2", recommend=10)
    exp = twin("kat", 0.3, 2)
    name = "asymmetricUserBasedModel"
    assert out["asym_user"] == {"alpha": 0.3, "q": 2, "frac_bits": None} and "asym" not in out
    assert list(out["mAP"])[-1] == name and len(out["mAP"]) == 6
    assert out["mAP"][name] == evaluation.threshold_map(exp, ds)
    lists = evaluation.rank_lists(exp, 10)[0]
    assert np.float64(out["mAP@K"][name]).view(np.int64) == \
        np.float64(rank_map_host(lists, 10, ds.lab_off, ds.lab_songs)[0]).view(np.int64)
    text = capsys.readouterr().out
    assert f"Elapsed time for {name} (alpha 0.3, q 2):\t" in text
    assert f"Elapsed time for {name} model mAP:\t" in text
    assert f"{name} model mAP: {driver.round_at(10, out['mAP'][name])}" in text
    assert f"{name} model mAP@10: {driver.round_at(10, out['mAP@K'][name])}" in text
    both = driver.run(ds.n_train, ds.n_test, str(tmp_path), asym=(0.15, 3), asym_user=(0.3, 2, 40), verbose=False)
    assert list(both["mAP"])[-2:] == ["asymmetricItemBasedModel", name] and len(both["mAP"]) == 7
    assert both["asym_user"]["frac_bits"] == 40
    assert both["mAP"][name] == evaluation.threshold_map(twin("kat", 0.3, 2, 40), ds)
