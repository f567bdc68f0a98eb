"""Full ranked lists, host side: evaluation.rank_lists (the numpy statement of
mr_rank_dense_device's order), mr_rank_merge_host, mr_rank_map_host and the
recommendation file round trip. No GPU."""
import ctypes
import functools

import numpy as np
import pytest

from musicrecommendation_amd import _lib, evaluation, modelio
from musicrecommendation_amd.engine import rank_map_host, rank_merge_host

from helpers import dataset_from_lines


def brute_rank(dense, K, song_lo=0):
    """Python's sort with an explicit comparator: value desc (-0.0 == +0.0),
    song asc; NaN skipped."""
    songs = np.full((dense.shape[0], K), -1, dtype=np.int32)
    scores = np.full((dense.shape[0], K), np.nan)

    def cmp(a, b):
        if a[0] != b[0]:
            return -1 if a[0] > b[0] else 1
        return a[1] - b[1]

    for u in range(dense.shape[0]):
        items = [(float(x), c + song_lo) for c, x in enumerate(dense[u].tolist()) if x == x]
        items.sort(key=functools.cmp_to_key(cmp))
        for i, (x, s) in enumerate(items[:K]):
            songs[u, i] = s
            scores[u, i] = x + 0.0
    return songs, scores


def same_lists(a, b):
    (sa, xa), (sb, xb) = a, b
    assert sa.dtype == np.int32 and xa.dtype == np.float64
    assert np.array_equal(sa, sb)
    assert np.array_equal(np.isnan(xa), np.isnan(xb))
    assert np.array_equal(np.isnan(xa), sa < 0)
    ok = ~np.isnan(xa)
    assert np.array_equal(xa[ok].view(np.int64), xb[ok].view(np.int64))


def matrices():
    rng = np.random.default_rng(11)
    rnd = rng.standard_normal((6, 97))
    rnd[rng.random(rnd.shape) < 0.2] = np.nan
    yield "random", rnd
    ties = rng.integers(-3, 4, size=(6, 97)) / 8.0
    ties[rng.random(ties.shape) < 0.2] = np.nan
    ties[2, ::2] = -0.0
    ties[2, 1::2] = 0.0
    ties[3] = np.nan
    ties[4] = 1.25
    ties[5, 3:] = np.nan
    ties[5, :3] = [-np.inf, np.inf, 5e-324]
    yield "ties", ties
    yield "f32", rng.integers(-3, 4, size=(4, 50)).astype(np.float32) / np.float32(3)


@pytest.mark.parametrize("K", [1, 5, 97, 200])
def test_rank_lists_is_the_brute_force_order(K):
    for name, m in matrices():
        same_lists(evaluation.rank_lists(m, K, song_lo=7), brute_rank(m, K, song_lo=7))
    s, x = evaluation.rank_lists(np.array([[-0.0, 0.0, np.nan, -1.0]]), 4)
    assert s.tolist() == [[0, 1, 3, -1]]
    assert not np.signbit(x[0, 0]) and x[0, 2] == -1.0 and np.isnan(x[0, 3])
    with pytest.raises(ValueError):
        evaluation.rank_lists(np.zeros(3), 2)


@pytest.mark.parametrize("K", [1, 5, 40, 200])
@pytest.mark.parametrize("cuts", [(), (48,), (31, 32), (1, 96)])
def test_merge_of_column_slices_is_the_whole(cuts, K):
    """1, 2 and 3 slices; the tie-heavy matrix has tie groups astride every cut,
    and short slices (and K > width) give lists padded with -1."""
    for name, m in matrices():
        if m.shape[1] < 97:
            continue
        bounds = [0, *cuts, m.shape[1]]
        parts = [evaluation.rank_lists(m[:, lo:hi], K, song_lo=lo) for lo, hi in zip(bounds, bounds[1:])]
        if K > min(hi - lo for lo, hi in zip(bounds, bounds[1:])):
            assert any((p[0] < 0).any() for p in parts)
        got = rank_merge_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
        same_lists(got, evaluation.rank_lists(m, K))


def test_merge_canonicalises_zero_and_skips_empty_slots():
    songs = np.array([[[4, -1, -1]], [[2, 9, -1]]], dtype=np.int32)
    scores = np.array([[[-0.0, np.nan, np.nan]], [[0.0, -np.inf, np.nan]]])
    s, x = rank_merge_host(songs, scores)
    assert s.tolist() == [[2, 4, 9]]
    assert not np.signbit(x[0, :2]).any() and x[0, 2] == -np.inf


def labelled(n_te, labels):
    """lab_off / lab_songs of n_te users from {user: [songs]}."""
    off = np.zeros(n_te + 1, dtype=np.int64)
    songs = []
    for u in range(n_te):
        songs += labels.get(u, [])
        off[u + 1] = len(songs)
    return off, np.array(songs, dtype=np.int32)


def fold_map(songs, k_eval, off, lab):
    """The issue's fold, written out: per user a left fold over the ranks, then
    a left fold over the users."""
    aps = []
    for u in range(songs.shape[0]):
        lset = set(lab[off[u]:off[u + 1]].tolist())
        a, h = 0.0, 0
        for i in range(1, k_eval + 1):
            s = int(songs[u, i - 1])
            hit = s >= 0 and s in lset
            if hit:
                h += 1
            a = a + (float(h) / float(i) if hit else 0.0)
        aps.append(a / float(min(k_eval, len(lset))) if lset else 0.0)
    total = 0.0
    for a in aps:
        total = total + a
    return (total / len(aps) if aps else 0.0), aps


class _Labels:  # what evaluation.map_at_k reads of a Dataset
    def __init__(self, n_te, off, lab):
        self.n_test, self.lab_off, self.lab_songs = n_te, off, lab


@pytest.mark.parametrize("k_eval", [1, 3, 10, 64, 300])
def test_map_host_fold_order_and_definition(k_eval):
    rng = np.random.default_rng(5)
    n_te, n_songs, K = 40, 400, 300
    songs = np.stack([rng.permutation(n_songs)[:K] for _ in range(n_te)]).astype(np.int32)
    songs[3, 100:] = -1            # a short list
    songs[4, :] = -1               # an empty one
    labels = {u: rng.integers(0, n_songs, size=rng.integers(1, 120)).tolist() for u in range(n_te)}
    labels[0] = []                                     # a user without labels
    labels[1] = [int(songs[1, 0])] * 3 + [int(songs[1, 2])]   # duplicates count once
    labels[2] = [int(songs[2, 1]), n_songs + 5, n_songs + 9]  # label-only ids count in n_u
    labels[5] = [n_songs + 1]                          # only a label-only id
    off, lab = labelled(n_te, labels)
    m, ap = rank_map_host(songs, k_eval, off, lab)
    em, eap = fold_map(songs, k_eval, off, lab)
    assert np.array_equal(ap.view(np.int64), np.array(eap).view(np.int64))
    assert np.float64(m).view(np.int64) == np.float64(em).view(np.int64)
    assert ap[0] == 0.0 and ap[4] == 0.0 and ap[5] == 0.0
    if k_eval >= 3:
        assert ap[1] == (1.0 + 2.0 / 3.0) / 2.0        # two distinct labels, hits at ranks 1 and 3
        assert ap[2] == 0.5 / 3.0                      # one hit at rank 2, n_u = 3
    # the vectorised definition sums in another order: <= 1024 terms <= 1
    assert abs(m - evaluation.map_at_k(songs, _Labels(n_te, off, lab), k=k_eval)) <= 1e-12


def test_map_host_no_users_and_dataset_labels():
    off = np.zeros(1, dtype=np.int64)
    m, ap = rank_map_host(np.zeros((0, 4), dtype=np.int32), 2, off, np.zeros(0, dtype=np.int32))
    assert m == 0.0 and ap.shape == (0,)
    ds = dataset_from_lines(["t\ta\t1", "t\tb\t1", "t\tc\t1"], ["x\ta\t1", "y\tb\t1"],
                            ["x\tb\t1", "x\tq\t1", "y\tc\t1"])
    si = {ds.song_names(i): i for i in range(ds.n_songs)}
    lists = np.array([[si["b"], -1], [si["a"], si["c"]]], dtype=np.int32)
    m, ap = rank_map_host(lists, 2, ds.lab_off, ds.lab_songs)
    assert ap.tolist() == [0.5, 0.5] and m == evaluation.map_at_k(lists, ds, k=2)


def test_host_calls_reject_bad_arguments():
    L = _lib.lib()
    s = np.zeros((1, 2, 4), dtype=np.int32)
    x = np.zeros((1, 2, 4))
    so, xo = np.zeros((2, 4), dtype=np.int32), np.zeros((2, 4))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.mr_rank_merge_host(1, 2, 4, p(s), p(x), p(so), p(xo)) == _lib.MR_OK
    assert L.mr_rank_merge_host(0, 2, 4, p(s), p(x), p(so), p(xo)) == _lib.MR_E_INVALID
    assert L.mr_rank_merge_host(1, -1, 4, p(s), p(x), p(so), p(xo)) == _lib.MR_E_INVALID
    assert L.mr_rank_merge_host(1, 2, 0, p(s), p(x), p(so), p(xo)) == _lib.MR_E_INVALID
    assert L.mr_rank_merge_host(1, 2, _lib.MR_RANK_MAX_K + 1, p(s), p(x), p(so), p(xo)) == _lib.MR_E_INVALID
    for bad in range(4):
        args = [p(s), p(x), p(so), p(xo)]
        args[bad] = None
        assert L.mr_rank_merge_host(1, 2, 4, *args) == _lib.MR_E_INVALID
    off, lab = labelled(2, {0: [1], 1: [2]})
    out = ctypes.c_double()
    ok = lambda **kw: L.mr_rank_map_host(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("n_te", 2), ("songs", p(so)), ("K", 4), ("k_eval", 4), ("off", p(off)), ("lab", p(lab)), ("ap", None),
        ("out", ctypes.byref(out)))])
    assert ok() == _lib.MR_OK
    assert ok(K=0) == _lib.MR_E_INVALID and ok(K=_lib.MR_RANK_MAX_K + 1, k_eval=1) == _lib.MR_E_INVALID
    assert ok(k_eval=0) == _lib.MR_E_INVALID and ok(k_eval=5) == _lib.MR_E_INVALID
    assert ok(n_te=-1) == _lib.MR_E_INVALID
    assert ok(songs=None) == _lib.MR_E_INVALID and ok(off=None) == _lib.MR_E_INVALID
    assert ok(out=None) == _lib.MR_E_INVALID
    bad_off = np.array([0, 2, 1], dtype=np.int64)
    assert ok(off=p(bad_off)) == _lib.MR_E_INVALID
    with pytest.raises(ValueError):
        rank_merge_host(np.zeros((2, 4), dtype=np.int32), np.zeros((2, 4)))
    with pytest.raises(_lib.EngineError):
        rank_map_host(so, 9, off, lab)


def test_recommendation_file_round_trip(tmp_path):
    recs = [("u1", [("s9", 0.1), ("s2", 1.0 / 3.0), ("s3", 5e-324), ("s4", -2.5e-7)]),
            ("u2", [("s1", 1e21), ("s7", float(np.float32(0.1))), ("s8", 0.0), ("s5", float("-inf"))])]
    path = str(tmp_path / "recs.txt")
    modelio.write_recommendations(path, recs)
    lines = open(path).read().splitlines()
    assert lines[0] == "u1\ts9\t0.1" and lines[4] == "u2\ts1\t1.0E21" and len(lines) == 8
    assert [l.split("\t")[0] for l in lines] == ["u1"] * 4 + ["u2"] * 4  # (user, rank) order
    back = modelio.read_recommendations(path)
    assert back == recs  # every score round-trips exactly
    with open(path, "a") as f:
        f.write("broken line\n")
    with pytest.raises(ValueError):
        modelio.read_recommendations(path)
