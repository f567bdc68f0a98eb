"""Similar-song queries on the device (csrc/mr_similar.hip):
mr_similar_songs_device against its numpy twin evaluation.song_similarity —
dense rows bit for bit, lists exactly (songs) and bitwise (scores) against
evaluation.similar_lists — on the fixtures with every song queried, across
song tiles and song shards, in every launch shape, on a hand-built dataset
whose counts pass 4,096 on two counters, against the engine's own
ItemBasedModel, and through the front ends."""
import os

import numpy as np
import pytest

from musicrecommendation_amd import _lib, driver, evaluation, modelio, synth
from musicrecommendation_amd.engine import Engine, rank_merge_host
from musicrecommendation_amd.ensemble import DeviceEnsemble
from musicrecommendation_amd.recommender import MusicRecommender

from helpers import GOLDEN, dataset_from_lines, kat, synth_fixture

pytestmark = pytest.mark.gpu

_twin = {}


def twin_rows(name, ds):
    """The twin's rows of every song, computed once per dataset."""
    if name not in _twin:
        _twin[name] = evaluation.song_similarity(ds, np.arange(ds.n_songs))
    return _twin[name]


def check_rows(rows, exp):
    got = rows.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(got[ok].view(np.int64), exp[ok].view(np.int64))
    return got


def check_lists(songs, scores, exp_rows, K, song_lo=0):
    songs, scores = songs.cpu().numpy(), scores.cpu().numpy()
    exp_songs, exp_scores = evaluation.similar_lists(exp_rows, K, song_lo=song_lo)
    assert songs.dtype == np.int32 and scores.dtype == np.float64
    assert np.array_equal(songs, exp_songs)
    assert np.array_equal(np.isnan(scores), exp_songs < 0)
    ok = exp_songs >= 0
    assert np.array_equal(scores[ok].view(np.int64), exp_scores[ok].view(np.int64))
    return songs, scores


def kat_dataset():
    K = kat()
    return dataset_from_lines(K["train"], K["test"], K["labels"])


@pytest.mark.parametrize("name", ["kat", "small"])
def test_fixtures_every_song_queried(name):
    ds = kat_dataset() if name == "kat" else synth_fixture("small")[0]
    exp = twin_rows(name, ds)
    q = np.arange(ds.n_songs)
    nonzero = np.count_nonzero(np.nan_to_num(exp), axis=1)
    with Engine(ds, out_dtype="f32") as e:  # the rows are fp64 whatever the context's out_dtype
        ens = DeviceEnsemble(e)
        for K in (1, 10, 64, 1024):
            songs, scores, rows = ens.similar_songs(q, K, dense=True)
            check_rows(rows, exp)
            got, _ = check_lists(songs, scores, exp, K)
            assert not (got == q[:, None]).any()  # the query itself is never listed
        assert (nonzero < 1024).mean() > 0.5 and (nonzero < 64).any()  # K exceeds the non-zero count of most rows
        assert np.array_equal((got >= 0).sum(axis=1), np.minimum(nonzero, 1024))
        rows0 = ens.similar_songs(q, 0, dense=True)[2]    # K = 0: rows only
        check_rows(rows0, exp)


def test_tiles_and_song_shards():
    ds, _ = synth_fixture("small")
    exp = twin_rows("small", ds)
    n = ds.n_songs
    rng = np.random.default_rng(5)
    q = np.concatenate([[0, 332, 333, 899, 900, n - 1], rng.integers(0, n, size=40)])  # in and out of every shard
    K = 20
    with Engine(ds, block_songs=256, stage1="separate") as e:
        assert e.block_songs == 256 and e.n_tiles == (n + 255) // 256 > 2 and n % 256 != 0
        one = check_lists(*DeviceEnsemble(e).similar_songs(q, K), exp[q], K)
    parts = []
    for lo, hi in ((0, 333), (333, 900), (900, n)):  # not tile-aligned
        with Engine(ds, block_songs=256, stage1="separate", song_lo=lo, song_hi=hi) as e:
            assert e.n_tiles > 1 and (e.song_lo, e.song_hi) == (lo, hi)
            songs, scores, rows = DeviceEnsemble(e).similar_songs(q, K, dense=True)
            check_rows(rows, exp[q][:, lo:hi])
            parts.append(check_lists(songs, scores, exp[q][:, lo:hi], K, song_lo=lo))
    m_songs, m_scores = rank_merge_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
    assert np.array_equal(m_songs, one[0])
    ok = one[0] >= 0
    assert np.array_equal(m_scores[ok].view(np.int64), one[1][ok].view(np.int64))
    assert np.isnan(m_scores[~ok]).all()


def test_song_sub_ranges_of_a_tile(monkeypatch):
    """A tile wider than the LDS counters is counted in song sub-ranges. No
    launch shape makes such a tile today (32,768 counters), so the capacity is
    lowered: tiles of 256 songs in passes of 100, 100 and 56."""
    ds, _ = synth_fixture("small")
    exp = twin_rows("small", ds)
    q = np.arange(0, ds.n_songs, 7)
    monkeypatch.setenv("MR_SIMILAR_COUNTERS", "100")
    with Engine(ds, block_songs=256, stage1="separate") as e:
        songs, scores, rows = DeviceEnsemble(e).similar_songs(q, 10, dense=True)
        check_rows(rows, exp[q])
        check_lists(songs, scores, exp[q], 10)


def test_every_launch_shape_gives_identical_bits():
    ds, _ = synth_fixture("small")
    exp = twin_rows("small", ds)
    q = np.arange(ds.n_songs)
    shapes = [("fused", dict(stage1="fused")),
              ("separate", dict(stage1="separate", topk=64)),
              ("wide", dict(stage1="wide", ibm_route="two_hop")),
              ("wide", dict(stage1="wide", ibm_route="cooc")),
              ("wide", dict(stage1="wide", train_order="given")),
              (None, dict(train_order="given"))]
    first = None
    for shape, kw in shapes:
        with Engine(ds, **kw) as e:
            assert shape is None or e.shape == shape
            if "ibm_route" in kw:
                assert e.ibm_route == kw["ibm_route"]
            songs, scores, rows = DeviceEnsemble(e).similar_songs(q, 10, dense=True)
            got = (check_rows(rows, exp),) + check_lists(songs, scores, exp, 10)
        if first is None:
            first = got
        else:
            assert np.array_equal(got[0].view(np.int64), first[0].view(np.int64))
            assert np.array_equal(got[1], first[1])
            assert np.array_equal(got[2].view(np.int64), first[2].view(np.int64))


N_HAND = 5000


def hand_dataset():
    """5,000 train users who all heard A and B plus one song of their own out of
    600 (S000..S599, user v hears S(v mod 600): 9 listeners for the first 200, 8
    for the others — whole groups of bitwise-equal cosines against A and B);
    ONE has a single train listener; TEST is heard by test users only."""
    train = []
    for v in range(N_HAND):
        train += [f"u{v:05d}\tA\t1", f"u{v:05d}\tB\t1", f"u{v:05d}\tS{v % 600:03d}\t1"]
    train.append("u00000\tONE\t1")
    test = ["x0\tTEST\t1", "x0\tA\t1", "x1\tTEST\t1", "x1\tS007\t1"]
    ds = dataset_from_lines(train, test, ["x0\tB\t1"])
    assert (ds.n_train, ds.n_songs) == (N_HAND, 604)
    return ds, {ds.song_names(i): i for i in range(ds.n_songs)}


def test_hand_built_heavy_counters_and_ties():
    ds, si = hand_dataset()
    q = np.array([si["A"], si["B"], si["TEST"], si["A"], si["ONE"], si["S007"]])
    exp = evaluation.song_similarity(ds, q)
    # the twin's own numbers, by hand
    assert exp[0, si["B"]] == N_HAND / (np.sqrt(np.float64(N_HAND + 1)) * np.sqrt(np.float64(N_HAND)))  # c(A) has x0's line
    assert exp[1, si["S000"]] == 9 / (np.sqrt(np.float64(N_HAND)) * np.sqrt(np.float64(9)))
    assert not exp[2][np.arange(ds.n_songs) != si["TEST"]].any()         # test listeners only: all zero
    assert np.count_nonzero(np.nan_to_num(exp[4])) == 3                   # u00000's A, B, S000
    a, b = si["S300"], si["S301"]
    assert exp[0, a].view(np.int64) == exp[0, b].view(np.int64) != 0      # a bitwise tie against A
    with Engine(ds, out_dtype="f64") as e:
        assert e.shape == "wide"  # chosen automatically at 5,000 train users
        ens = DeviceEnsemble(e)
        for K in (10, 1024):
            songs, scores, rows = ens.similar_songs(q, K, dense=True)
            check_rows(rows, exp)
            ls, _ = check_lists(songs, scores, exp, K)
        assert (ls[2] == -1).all()                                         # empty list
        assert np.array_equal(ls[0], ls[3])                                # the repeated query
        row = ls[0].tolist()
        assert row.index(a) + 1 == row.index(b)                            # ties in song-id order
        assert sorted(ls[4][ls[4] >= 0].tolist()) == sorted([si["A"], si["B"], si["S000"]])
        # n_q = 0: succeeds, nothing written
        import torch

        keep = torch.full((4,), -7, dtype=torch.int32, device=ens.device)
        e.similar_songs(np.zeros(0, dtype=np.int32), 4, keep.data_ptr())
        assert (keep.cpu().numpy() == -7).all()
        empty = ens.similar_songs([], 4)
        assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0, 4)


def test_rows_sum_to_the_engines_item_based_model():
    """Σ_{s2 ∈ T(u)} cos(s, s2) is rank(u, s) (MR:249-257): the device rows
    against the engine's own fixed-point ItemBasedModel, within the project's
    literal-vs-fixed-point bound 1e-7 (DESIGN §2 measured <= 5e-9)."""
    ds = synth.config("c1").dataset()
    with Engine(ds, out_dtype="f64") as e:
        ibm = e.score_dense("ibm")
        ens = DeviceEnsemble(e)
        busiest = np.argsort(-np.count_nonzero(np.nan_to_num(ibm), axis=1), kind="stable")[:3]
        for u in busiest.tolist():  # the three users whose engine rows hold the most non-zero pairs
            heard = np.asarray(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]])
            rows = ens.similar_songs(heard, 0, dense=True)[2].cpu().numpy()
            out = np.ones(ds.n_songs, dtype=bool)
            out[heard] = False
            assert np.isnan(ibm[u, heard]).all() and not np.isnan(rows[:, out]).any()
            total = rows[:, out].sum(axis=0)  # cos is symmetric: column s of the rows of T(u)
            ref = ibm[u, out]
            err = np.abs(total - ref)
            print(f"user {u}: max relative error {np.max(err / np.maximum(np.abs(ref), 1e-300)):.3e}")
            assert (err <= 1e-7 * np.abs(ref)).all() and np.count_nonzero(ref) > 0


def test_errors_leave_the_outputs_untouched():
    import torch

    ds = kat_dataset()
    with Engine(ds) as e:
        ens = DeviceEnsemble(e)
        songs = torch.full((2, 3), -7, dtype=torch.int32, device=ens.device)
        scores = torch.full((2, 3), 2.5, dtype=torch.float64, device=ens.device)
        rows = torch.full((2, e.width), 2.5, dtype=torch.float64, device=ens.device)
        for bad in ([0, ds.n_songs], [-1, 0]):
            with pytest.raises(_lib.EngineError) as ei:
                e.similar_songs(bad, 3, songs.data_ptr(), scores.data_ptr(), rows.data_ptr())
            assert ei.value.code == _lib.MR_E_INVALID
        torch.cuda.synchronize()
        assert (songs == -7).all() and (scores == 2.5).all() and (rows == 2.5).all()
        with pytest.raises(_lib.EngineError) as ei:
            e.similar_songs([0], 0, songs.data_ptr())  # K = 0 without dense_dev
        assert ei.value.code == _lib.MR_E_INVALID
        with pytest.raises(_lib.EngineError) as ei:
            e.similar_songs([0], 3, 0, 0, rows.data_ptr())  # K >= 1 without songs_dev
        assert ei.value.code == _lib.MR_E_INVALID
        with pytest.raises(_lib.EngineError):
            e.similar_songs([0], _lib.MR_RANK_MAX_K + 1, songs.data_ptr())
        e.similar_songs([0, 1], 3, songs.data_ptr())  # scores_dev may be NULL
        assert (scores == 2.5).all() and not (songs == -7).any()


def test_recommender_similar_songs_and_explain():
    K = kat()
    ds = kat_dataset()
    exp = twin_rows("kat", ds)
    names = [ds.song_names(i) for i in range(ds.n_songs)]
    rec = MusicRecommender(K["train"], K["test"], K["labels"])
    try:
        order = names[::-1] + names[:1]
        got = rec.similarSongs(order, K=3)
        qi = [names.index(n) for n in order]
        e_songs, e_scores = evaluation.similar_lists(exp[qi], 3)
        assert [g[0] for g in got] == order
        for i, (_name, items) in enumerate(got):
            n = int((e_songs[i] >= 0).sum())
            assert [s for s, _ in items] == [names[j] for j in e_songs[i, :n]]
            assert [x for _, x in items] == e_scores[i, :n].tolist()
        assert any(items for _n, items in got)
        with pytest.raises(KeyError):
            rec.similarSongs(["no such song"])
        checked = 0
        for u in range(ds.n_test):
            heard = ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]].tolist()
            for s in range(ds.n_songs):
                if s in heard:
                    with pytest.raises(ValueError):
                        rec.explain(ds.test_names(u), names[s])
                    continue
                terms = rec.explain(ds.test_names(u), names[s])
                want = sorted(((names[s2], float(exp[s, s2])) for s2 in heard if exp[s, s2] != 0),
                              key=lambda t: (-t[1], t[0]))
                assert terms == want
                checked += len(terms)
        assert checked > 0
        with pytest.raises(KeyError):
            rec.explain("nobody", names[0])
    finally:
        rec.close()


def test_driver_similar(tmp_path, capsys):
    z = np.load(os.path.join(GOLDEN, "synth_small.npz"))
    n_tr = len({l.split("\t")[0] for l in z["train"].tolist()})
    n_te = len({l.split("\t")[0] for l in z["test"].tolist()})
    for key, fn in (("train", "train"), ("test", "test"), ("labels", "test_labels")):
        (tmp_path / f"{fn}_{n_tr}_{n_te}.txt").write_text("".join(l + "\n" for l in z[key].tolist()))
    path = str(tmp_path / "similar.txt")
    out = driver.run(n_tr, n_te, str(tmp_path), similar=(5, path))
    ds, _ = synth_fixture("small")
    q = np.unique(ds.te_songs)
    assert out["similar"] == {"K": 5, "path": path, "queries": int(q.size)}
    text = capsys.readouterr().out
    assert f"similar-song queries: {q.size}" in text and f"Elapsed time for top-5 similar songs of {q.size} songs:" in text
    e_songs, e_scores = evaluation.similar_lists(twin_rows("small", ds)[q], 5)
    want = [(ds.song_names(int(s)), [(ds.song_names(int(g)), float(x)) for g, x in zip(e_songs[i], e_scores[i]) if g >= 0])
            for i, s in enumerate(q)]
    assert modelio.read_recommendations(path) == [w for w in want if w[1]]  # exact: the scores round-trip
