"""Full ranked recommendation lists on the device (csrc/mr_rank.hip):
mr_rank_dense_device against evaluation.rank_lists (songs exactly, scores
bitwise) on hand-built dense models that aim at the radix select's paths — the
whole row in the candidate buffer, a bucket that fits after one or more digits,
and a tie group larger than the buffer, where the select runs to the last digit
and keeps the lowest song ids —, song shards merged by mr_rank_merge_host, real
models, the truncated mAP on the device, and the front ends."""
import ctypes

import numpy as np
import pytest

from musicrecommendation_amd import _lib, driver, evaluation, modelio
from musicrecommendation_amd.engine import Engine, rank_map_host, rank_merge_host
from musicrecommendation_amd.ensemble import DeviceEnsemble
from musicrecommendation_amd.recommender import MusicRecommender

import topk_cases as tc
from helpers import dataset_from_lines, kat, synth_fixture

pytestmark = pytest.mark.gpu

KS = [1, 10, 64, 500, 1024]
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
_cache = {}


def wide_dataset(n_songs, n_users):
    """n_users test users x n_songs songs, every pair unheard but the anchor's
    (the models are hand-made: only the shape matters)."""
    key = (n_songs, n_users)
    if key not in _cache:
        train = [f"t\t{tc.song(s)}\t1" for s in range(n_songs - 1)] + [f"t\t{tc.ANCHOR}\t1"]
        test = [f"x{u}\t{tc.ANCHOR}\t1" for u in range(n_users)]
        _cache[key] = dataset_from_lines(train, test, [f"x0\t{tc.song(0)}\t1"])
        assert (_cache[key].n_test, _cache[key].n_songs) == (n_users, n_songs)
    return _cache[key]


def check_lists(got_songs, got_scores, model, K, song_lo=0):
    """Device lists == evaluation.rank_lists of the host copy: songs exactly,
    scores bitwise, NaN in the empty slots."""
    songs, scores = got_songs.cpu().numpy(), got_scores.cpu().numpy()
    exp_songs, exp_scores = evaluation.rank_lists(model, K, song_lo=song_lo)
    assert songs.dtype == np.int32 and scores.dtype == np.float64
    assert np.array_equal(songs, exp_songs)
    assert np.array_equal(np.isnan(scores), exp_songs < 0)
    ok = exp_songs >= 0
    assert np.array_equal(scores[ok].view(np.int64), exp_scores[ok].view(np.int64))
    return songs, scores


def rank_and_check(ens, model, K, song_lo=0):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(model)).to(ens.device)
    return check_lists(*ens.rank(t, K), model, K, song_lo=song_lo)


def hand_models(dtype, w=2301):
    """Two 5-row models of the hand-built rows."""
    rng = np.random.default_rng(3)
    ft = NP_DTYPE[dtype]
    tiny = np.finfo(ft).smallest_subnormal
    a = np.empty((5, w), dtype=ft)
    a[0] = rng.integers(0, 40, size=w) / 8.0                       # integer eighths, heavy ties
    a[1] = rng.random(w) * 0.5                                     # 40 equal maxima, then a 100-strong group:
    a[1, rng.choice(w, 140, replace=False)[:40]] = 7.0             # the K = 10 cut falls inside the first,
    second = np.flatnonzero(a[1] < 7.0)[5::17][:100]
    a[1, second] = 3.0                                             # the K = 64 cut inside the second
    a[2] = 0.375                                                   # one constant row
    a[3] = np.where(rng.random(w) < 0.5, 0.0, -0.0)                # +0.0 / -0.0 only
    a[4] = np.nan                                                  # all NaN
    b = np.empty((5, w), dtype=ft)
    b[0] = np.nan
    b[0, [2, 1150, w - 1]] = [0.5, 0.5, -1.0]                      # three valid entries
    b[1] = rng.integers(-20, 21, size=w) / 4.0                     # negative, zero, positive, +-inf
    b[1, rng.choice(w, 30, replace=False)] = np.repeat([np.inf, -np.inf, 0.0], 10)
    b[2] = (rng.integers(-6, 7, size=w) * tiny).astype(ft)         # denormals next to zero
    b[2, ::7] = -0.0
    b[3] = rng.standard_normal(w)
    b[3, ::3] = np.nan                                             # every third entry NaN
    b[4] = -np.abs(rng.standard_normal(w)) * 1e-3                  # all negative
    assert np.count_nonzero(a[1] == 7.0) == 40 and np.count_nonzero(a[1] == 3.0) == 100
    assert np.count_nonzero((b[2] != 0) & (np.abs(b[2]) < np.finfo(ft).tiny)) > 1000  # denormals survived
    return a, b


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_hand_built_rows(dtype):
    ds = wide_dataset(2301, 5)
    with Engine(ds, out_dtype=dtype) as e:
        ens = DeviceEnsemble(e)
        for model in hand_models(dtype):
            for K in KS:
                songs, scores = rank_and_check(ens, model, K)
        # (the last model's last K) -0.0 is returned as +0.0
        a = hand_models(dtype)[0]
        songs, scores = rank_and_check(ens, a, 1024)
        assert not np.signbit(scores[3]).any() and songs[3].tolist() == list(range(1024))
        assert (songs[4] == -1).all()


def wide_models(dtype, w=40001):
    rng = np.random.default_rng(9)
    ft = NP_DTYPE[dtype]
    a = np.empty((3, w), dtype=ft)
    a[0] = 2.5                                   # constant: a tie group beyond any candidate buffer
    a[1] = np.where(np.arange(w) % 2 == 1, 1.0, 0.25)   # more than K of the upper value
    a[2] = 0.25
    a[2, 11::137][:290] = 1.0                    # fewer than K of the upper value: the cut is in the lower ties
    b = np.empty((3, w), dtype=ft)
    it = {"f32": (np.uint32, 10), "f64": (np.uint64, 20)}[dtype]
    base = np.array([1.5], dtype=ft).view(it[0])[0]
    low = rng.integers(0, 1 << it[1], size=w).astype(it[0])
    b[0] = (base | low).view(ft)                 # equal but for the low mantissa bits: the last radix digits decide
    b[1] = -2.5                                  # a negative constant
    b[2] = rng.standard_normal(w)
    b[2, ::5] = np.nan
    assert np.count_nonzero(a[2] == 1.0) == 290
    return a, b


@pytest.mark.parametrize("K", [500, 1024])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_wide_odd_width_rows(dtype, K):
    """40,001 columns: f32 rows 1 and 2 start 4-byte aligned only."""
    ds = wide_dataset(40001, 3)
    with Engine(ds, out_dtype=dtype) as e:
        ens = DeviceEnsemble(e)
        a, b = wide_models(dtype)
        songs, scores = rank_and_check(ens, a, K)
        assert songs[0].tolist() == list(range(K))                  # the K lowest song ids of the tie
        assert songs[1].tolist() == list(range(1, 2 * K, 2))
        assert (scores[2, :290] == 1.0).all() and (scores[2, 290:] == 0.25).all()
        songs, scores = rank_and_check(ens, b, K)
        assert songs[1].tolist() == list(range(K))
        # the hand-built rows at this width, where the radix select (not the whole-row sort) picks them
        ha, hb = hand_models(dtype, 40001)
        rows = np.concatenate([ha, hb, ha[:2]])
        for i in range(0, rows.shape[0], 3):
            rank_and_check(ens, rows[i:i + 3], K)


@pytest.mark.parametrize("K", [500, 1024])
@pytest.mark.parametrize("width", [1, 63, 64, 65, 1025])
def test_narrow_shards_are_padded(width, K):
    """Contexts of narrow song ranges (song_lo > 0): short lists padded with -1."""
    ds = wide_dataset(2301, 5)
    lo = 130
    for dtype in ("f32", "f64"):
        model = hand_models(dtype)[1][:, lo:lo + width]
        with Engine(ds, out_dtype=dtype, song_lo=lo, song_hi=lo + width) as e:
            songs, scores = rank_and_check(DeviceEnsemble(e), model, K, song_lo=lo)
            n_valid = np.count_nonzero(~np.isnan(model), axis=1)
            assert np.array_equal(np.count_nonzero(songs >= 0, axis=1), np.minimum(n_valid, K))
            assert songs[songs >= 0].min() >= lo and songs.max() < lo + width


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_song_shards_merge_to_the_one_context_lists(dtype):
    import torch

    ds = wide_dataset(2301, 5)
    models = hand_models(dtype)
    with Engine(ds, out_dtype=dtype) as e:
        ens = DeviceEnsemble(e)
        whole = {(m, K): [x.cpu().numpy() for x in ens.rank(torch.from_numpy(models[m]).to(ens.device), K)]
                 for m in range(2) for K in (10, 500, 1024)}
    # uneven cuts; column 1 and 700 lie inside the constant row's (and the eighths') tie groups
    for bounds in ([0, 700, 2301], [0, 1, 1500, 2301]):
        parts = {}
        for lo, hi in zip(bounds, bounds[1:]):
            with Engine(ds, out_dtype=dtype, song_lo=lo, song_hi=hi) as e:
                ens = DeviceEnsemble(e)
                for (m, K) in whole:
                    t = torch.from_numpy(np.ascontiguousarray(models[m][:, lo:hi])).to(ens.device)
                    parts.setdefault((m, K), []).append([x.cpu().numpy() for x in ens.rank(t, K)])
        for key, lists in parts.items():
            songs, scores = rank_merge_host(np.stack([p[0] for p in lists]), np.stack([p[1] for p in lists]))
            assert np.array_equal(songs, whole[key][0]), (bounds, key)
            assert np.array_equal(scores.view(np.int64), whole[key][1].view(np.int64)), (bounds, key)


def real_datasets():
    K = kat()
    yield "kat", dataset_from_lines(K["train"], K["test"], K["labels"])
    yield "small", synth_fixture("small")[0]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_real_models(dtype):
    negatives = 0
    for name, ds in real_datasets():
        with Engine(ds, out_dtype=dtype, topk=10) as e:
            ens = DeviceEnsemble(e)
            ubm, ibm = ens.model("ubm"), ens.model("ibm")
            models = {"ubm": ubm, "ibm": ibm, "linear 0.5": ens.linear(ubm, ibm, 0.5),
                      "linear 1.5": ens.linear(ubm, ibm, 1.5)}
            negatives += int((models["linear 1.5"].cpu().numpy() < 0).sum())
            for mname, t in models.items():
                host = t.cpu().numpy()
                for K in (10, 500):
                    songs, scores = check_lists(*ens.rank(t, K), host, K)
                if dtype == "f64" and not (host < 0).any():
                    top_songs, top_scores, _keys = ens.topk(t)
                    k10 = evaluation.rank_lists(host, 10)
                    assert np.array_equal(top_songs, k10[0]), (name, mname)
                    assert np.array_equal(top_scores[k10[0] >= 0], k10[1][k10[0] >= 0]), (name, mname)
    assert negatives > 0  # alpha outside [0, 1]: negative scores were ranked


def test_map_on_device_equals_host_fold():
    ds, z = synth_fixture("small")
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        for t in (ens.model("ubm"), ens.model("ibm")):
            lists = ens.rank(t, 500)
            host_songs = lists[0].cpu().numpy()
            for k_eval in (1, 10, 500):
                m_dev, ap_dev = e.rank_map(lists[0].data_ptr(), 500, k_eval, ds.lab_off, ds.lab_songs)
                m_host, ap_host = rank_map_host(host_songs, k_eval, ds.lab_off, ds.lab_songs)
                print(f"k_eval={k_eval}: device {m_dev!r} host {m_host!r} "
                      f"numpy {evaluation.map_at_k(host_songs, ds, k=k_eval)!r}")
                assert np.array_equal(ap_dev.view(np.int64), ap_host.view(np.int64))
                assert np.float64(m_dev).view(np.int64) == np.float64(m_host).view(np.int64)
                assert abs(m_dev - evaluation.map_at_k(host_songs, ds, k=k_eval)) <= 1e-12
                assert ens.map_at(lists, k_eval) == m_dev and ens.map_at(lists[0], k_eval) == m_dev
            assert ens.map_at(t, 10, K=500) == ens.map_at(lists, 10)
            assert ens.map_at(t, 10) == ens.map_at(lists, 10)  # ranked at K = 10: the same first ten
            assert ens.map_at(lists, 500) > 0.0


def test_rank_is_ordered_after_pending_torch_work():
    ds = wide_dataset(40001, 3)
    with Engine(ds, out_dtype="f32") as e:
        import torch

        ens = DeviceEnsemble(e)
        t = torch.from_numpy(wide_models("f32")[1]).to(ens.device)
        torch.cuda.synchronize()
        for _ in range(3):
            got = ens.rank(t * 2 + 1, 500)  # no sync between the torch expression and the engine's stream
            check_lists(*got, (t * 2 + 1).cpu().numpy(), 500)


def test_argument_errors_launch_nothing():
    import torch

    ds = wide_dataset(2301, 5)
    with Engine(ds, out_dtype="f64") as e:
        ens = DeviceEnsemble(e)
        t = torch.zeros(ens.shape, dtype=torch.float64, device=ens.device)
        songs = torch.full((5, 1024), 77, dtype=torch.int32, device=ens.device)
        scores = torch.full((5, 1024), 77.0, dtype=torch.float64, device=ens.device)
        torch.cuda.synchronize()
        for K in (0, -3, 1025):
            with pytest.raises(_lib.EngineError) as ei:
                e.rank_dense(t.data_ptr(), K, songs.data_ptr(), scores.data_ptr())
            assert ei.value.code == _lib.MR_E_INVALID
            with pytest.raises(_lib.EngineError):
                ens.rank(t, K)
        for args in ((0, 10, songs.data_ptr(), scores.data_ptr()), (t.data_ptr(), 10, 0, scores.data_ptr())):
            with pytest.raises(_lib.EngineError) as ei:
                e.rank_dense(*args)
            assert ei.value.code == _lib.MR_E_INVALID
        with pytest.raises(_lib.EngineError) as ei:
            e.rank_map(0, 10, 10, ds.lab_off, ds.lab_songs)
        assert ei.value.code == _lib.MR_E_INVALID
        with pytest.raises(_lib.EngineError) as ei:
            e.rank_map(songs.data_ptr(), 10, 11, ds.lab_off, ds.lab_songs)
        assert ei.value.code == _lib.MR_E_INVALID
        # before mr_load: MR_E_STATE (valid buffers all the same)
        L = _lib.lib()
        opt = _lib.MrOptions()
        _lib.check(L.mr_options_default(ctypes.byref(opt)), "mr_options_default")
        h = ctypes.c_void_p()
        _lib.check(L.mr_create(ctypes.byref(opt), ctypes.byref(h)), "mr_create")
        try:
            assert L.mr_rank_dense_device(h, t.data_ptr(), 10, songs.data_ptr(), scores.data_ptr()) == _lib.MR_E_STATE
            out = ctypes.c_double()
            off = np.ascontiguousarray(ds.lab_off, dtype=np.int64)
            lab = np.ascontiguousarray(ds.lab_songs, dtype=np.int32)
            assert L.mr_rank_map_device(h, songs.data_ptr(), 10, 10, off.ctypes.data_as(ctypes.c_void_p),
                                        lab.ctypes.data_as(ctypes.c_void_p), None,
                                        ctypes.byref(out)) == _lib.MR_E_STATE
        finally:
            L.mr_destroy(h)
        torch.cuda.synchronize()
        assert (songs == 77).all() and (scores == 77.0).all()  # nothing ran
        e.rank_dense(t.data_ptr(), 10, songs.data_ptr(), 0)     # scores may be NULL
        assert songs.view(-1)[:50].view(5, 10).cpu().tolist() == [list(range(10))] * 5
        assert (scores == 77.0).all()


def _kat_resources(tmp_path):
    K = kat()
    n_tr = len({l.split("\t")[0] for l in K["train"]})
    n_te = len({l.split("\t")[0] for l in K["test"]})
    paths = []
    for key, fn in (("train", "train"), ("test", "test"), ("labels", "test_labels")):
        p = tmp_path / f"{fn}_{n_tr}_{n_te}.txt"
        p.write_text("".join(l + "\n" for l in K[key]))
        paths.append(str(p))
    return n_tr, n_te, paths


def test_driver_recommend_and_recommender(tmp_path, capsys):
    n_tr, n_te, paths = _kat_resources(tmp_path)
    plain = driver.run(n_tr, n_te, str(tmp_path), verbose=False)
    assert set(plain) == {"mAP", "multi_gpu_checked", "thresholds", "layout"}
    plain_text = capsys.readouterr().out
    assert "mAP@" not in plain_text
    out_path = str(tmp_path / "recs.txt")
    out = driver.run(n_tr, n_te, str(tmp_path), verbose=False, recommend=f"500:{out_path}")
    text = capsys.readouterr().out
    assert text.startswith(plain_text)  # the flow's own output is unchanged
    assert set(out) == set(plain) | {"mAP@K", "recommend"} and out["mAP"] == plain["mAP"]
    assert list(out["mAP@K"]) == list(out["mAP"]) and out["recommend"] == {"K": 500, "path": out_path}
    for name, v in out["mAP@K"].items():
        assert f"{name} model mAP@500: {driver.round_at(10, v)}" in text
    mr = MusicRecommender(*paths)
    try:
        ubm = mr.sorted_model(mr.getUserBasedModel())
        ibm = mr.sorted_model(mr.getItemBasedModel())
        lcm = mr.getLinearCombinationModel(ubm, ibm, 0.5)
        recs = mr.recommend(lcm, K=500)
        assert [u for u, _ in recs] == [mr.dataset.test_names(u) for u in range(mr.dataset.n_test)]
        assert all(items for _, items in recs)
        assert modelio.read_recommendations(out_path) == recs
        assert mr.evaluateRanking(lcm, k=500) == out["mAP@K"]["linear-combination"]
        assert mr.evaluateRanking("ubm", k=500) == out["mAP@K"]["user-based"]
        top3 = mr.recommend("ubm", K=3)
        dense = mr.scores("ubm")
        exp = evaluation.rank_lists(dense, 3)
        for u, (user, items) in enumerate(top3):
            n = int((exp[0][u] >= 0).sum())
            assert [s for s, _ in items] == [mr.dataset.song_names(int(g)) for g in exp[0][u, :n]]
            assert [x for _, x in items] == exp[1][u, :n].tolist()
    finally:
        mr.close()
    assert driver.main([str(n_tr), str(n_te), "--resources", str(tmp_path), "--quiet", "--recommend", "5"]) == 0
    assert "user-based model mAP@5:" in capsys.readouterr().out
    with pytest.raises(ValueError):
        driver.run(n_tr, n_te, str(tmp_path), verbose=False, recommend="2000")
