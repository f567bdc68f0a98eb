"""The edges of the shared tile walk (csrc/mr_tile_walk.h) at the smallest
shapes that reach them, in every kernel that instantiates it: the similar-song
counts, the asymmetric item-based and user-based models, the two-hop scoring
and the co-listening index build. The fixtures' listener lists are short: none
runs a third iteration of the software pipeline in a 1024-thread kernel.

One hand-built dataset: 6,200 train users, 3 test users, 300 songs in tiles of
256 (the smallest tile; the second one holds 44 songs). Song LISTENERS[s] is
heard by the train users 0 .. k-1 for k = 0, 1, 1024, 1025, 2047, 2048, 2049,
4096, 4097 and 6145: with 2 listeners per thread and 1024 threads an iteration
of the walk covers 2048 entries, so the lists take 0, 1, 2, 3 and 4 iterations
and sit on both sides of every boundary of the i+1 / i+2 prefetch. A few filler
songs give the listeners' per-tile segments the lengths 0, 1, 3, 4, 5, 8 and 9
around the 4 ids a segment's head loads together. Every result is compared bit
for bit with its numpy twin or the fixed-point oracle, plain and with the
sub-ranges lowered to 64 songs (16 train users per chunk), so that a sub-range
boundary (songs 64, 128, 192) falls inside a segment."""
import numpy as np
import pytest

from musicrecommendation_amd import evaluation
from musicrecommendation_amd.dataset import Dataset
from musicrecommendation_amd.engine import Engine
from musicrecommendation_amd.ensemble import DeviceEnsemble

gpu = pytest.mark.gpu

N_TRAIN, N_SONGS, TILE = 6200, 300, 256
LISTENERS = {10: 0, 62: 1, 63: 1024, 64: 1025, 65: 2047, 130: 2048, 200: 2049, 256: 4096, 257: 4097, 290: 6145}
# (first user, last user + 1, songs): fillers on top of the prefix songs above
FILLERS = [(100, 200, (20, 21, 22, 23)), (200, 300, (20, 21, 22)),               # tile 0: 5 + 4 and 5 + 3 ids
           (300, 400, (260, 261, 262, 263, 264, 265)), (400, 500, (260, 261, 262, 263, 264)),  # tile 1: 3 + 6, 3 + 5
           (6145, N_TRAIN, (5,))]                                                  # the users past every prefix
TEST = {10000: (10, 62, 63, 64, 200, 257), 10001: (23, 65, 130, 256, 290)}         # 10002: every song nobody else hears
SEGMENT_LENGTHS = {0, 1, 3, 4, 5, 8, 9}
QUERIES = np.array(sorted(LISTENERS) + [20, 265], dtype=np.int32)
GRID = [(0.5, 1), (0.15, 3)]
SMALL = {"MR_SIMILAR_COUNTERS": "64", "MR_ASYM_SUB": "64", "MR_UASYM_SUB": "64", "MR_UASYM_CHUNK": "16"}
ENV = tuple(SMALL) + ("MR_UASYM_BATCH", "MR_LAUNCH_ROWS")

_cache = {}


def dataset():
    if "ds" not in _cache:
        tu, ts = [], []
        for s, k in LISTENERS.items():
            tu.append(np.arange(k))
            ts.append(np.full(k, s))
        for lo, hi, songs in FILLERS:
            for s in songs:
                tu.append(np.arange(lo, hi))
                ts.append(np.full(hi - lo, s))
        tu, ts = np.concatenate(tu), np.concatenate(ts)
        used = set(ts.tolist()) | {s for songs in TEST.values() for s in songs}
        test = dict(TEST)
        test[10002] = tuple(s for s in range(N_SONGS) if s not in used) + (20,)
        eu = np.concatenate([np.full(len(v), u) for u, v in test.items()])
        es = np.concatenate([np.asarray(v) for v in test.values()])
        ds = Dataset.from_triplets(tu, ts, eu, es, np.array([10000, 10001]), np.array([130, 63]))
        assert (ds.n_train, ds.n_test, ds.n_songs) == (N_TRAIN, 3, N_SONGS)  # song id = song key
        _cache["ds"] = ds
    return _cache["ds"]


def twin(kind, *args):
    """A twin's result, computed once and never written to."""
    key = (kind,) + args
    if key not in _cache:
        ds = dataset()
        if kind == "similar":
            t = evaluation.song_similarity(ds, QUERIES)
        elif kind == "item":
            t = evaluation.asym_item_model(ds, *args)
        elif kind == "user":
            t = evaluation.asym_user_model(ds, *args, 32)
        else:
            from oracle import native
            t = native.fp_model(ds, "ibm", frac_bits=32, k=10)
            for a in t:
                a.setflags(write=False)
        if kind != "ibm":
            t.setflags(write=False)
        _cache[key] = t
    return _cache[key]


def test_the_dataset_holds_the_list_and_segment_lengths():
    ds = dataset()
    assert -(-ds.n_songs // TILE) == 2 and ds.n_songs % TILE != 0  # two tiles, the last one partial
    users = np.repeat(np.arange(ds.n_train), np.diff(ds.tr_off))
    songs = np.asarray(ds.tr_songs)
    count = np.bincount(songs, minlength=ds.n_songs)
    assert {int(count[s]) for s in LISTENERS} == {0, 1, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 6145}
    assert all(int(count[s]) == k for s, k in LISTENERS.items())
    heard = set(np.asarray(ds.te_songs).tolist())
    assert set(LISTENERS) <= heard and set(LISTENERS) <= set(QUERIES.tolist())  # each is a query and a heard song
    # segment lengths of the listeners of the query songs, per tile
    seg = np.zeros((2, ds.n_train), dtype=np.int64)
    np.add.at(seg, (songs // TILE, users), 1)
    listeners = np.unique(users[np.isin(songs, QUERIES)])
    assert SEGMENT_LENGTHS <= set(seg[0, listeners].tolist())
    assert {1, 2, 3, 8, 9} <= set(seg[1, listeners].tolist())
    # a segment head that straddles the sub-range boundaries at songs 64 and 128
    row = songs[ds.tr_off[1]:ds.tr_off[2]].tolist()
    assert row[:4] == [63, 64, 65, 130]


def check(got, exp):
    """NaN in the same places, every other value bit-equal."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == np.float64 and got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(got[ok].view(np.int64), exp[ok].view(np.int64))
    return got


@pytest.fixture(scope="module")
def engine():
    with Engine(dataset(), out_dtype="f64", topk=10, frac_bits=32, stage1="wide", ibm_route="two_hop",
                block_songs=TILE) as e:
        assert e.shape == "wide" and e.ibm_route == "two_hop" and (e.block_songs, e.n_tiles) == (TILE, 2)
        yield e


@pytest.fixture(params=["plain", "small"])
def sub_ranges(request, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if request.param == "small":
        for name, value in SMALL.items():
            monkeypatch.setenv(name, value)
    return request.param


@gpu
def test_similar_songs(engine, sub_ranges):
    exp = twin("similar")
    assert np.count_nonzero(np.nan_to_num(exp[QUERIES.tolist().index(290)])) > 10
    songs, scores, rows = DeviceEnsemble(engine).similar_songs(QUERIES, 5, dense=True)
    check(rows, exp)
    e_songs, e_scores = evaluation.similar_lists(exp, 5)
    songs, scores = songs.cpu().numpy(), scores.cpu().numpy()
    assert np.array_equal(songs, e_songs)
    ok = e_songs >= 0
    assert np.array_equal(scores[ok].view(np.int64), e_scores[ok].view(np.int64))
    assert np.isnan(scores[~ok]).all()
    assert (songs[QUERIES.tolist().index(10)] == -1).all()  # no train listener: an empty list


@gpu
@pytest.mark.parametrize("alpha,q", GRID)
def test_asymmetric_item_model(engine, sub_ranges, alpha, q):
    exp = twin("item", alpha, q)
    got = check(DeviceEnsemble(engine).item_based(alpha, q), exp)
    assert np.array_equal(np.isnan(got), dataset().heard_mask())
    assert np.count_nonzero(np.nan_to_num(got), axis=1).min() > 0


@gpu
@pytest.mark.parametrize("alpha,q", GRID)
def test_asymmetric_user_model(engine, sub_ranges, alpha, q):
    exp = twin("user", alpha, q)
    got = check(DeviceEnsemble(engine).user_based(alpha, q), exp)
    assert np.array_equal(np.isnan(got), dataset().heard_mask())
    assert np.count_nonzero(np.nan_to_num(got), axis=1).min() > 0
    if (alpha, q) == (0.5, 1):  # the engine's own UserBasedModel, bit for bit
        check(got, engine.score_dense("ubm"))


def check_ibm(e):
    exp, ts, tk = twin("ibm")
    got = e.score_dense("ibm")
    songs, _scores, keys = e.topk()
    assert np.array_equal(got, exp, equal_nan=True), "dense scores differ from the fixed-point oracle"
    assert np.array_equal(songs, ts) and np.array_equal(keys, tk), "top-k differs from the fixed-point oracle"


@gpu
def test_item_based_model_two_hop(engine):
    check_ibm(engine)


@gpu
@pytest.mark.parametrize("build", ["default", "pertile"])
def test_item_based_model_co_listening(build, monkeypatch):
    """The co-listening route forced; `pertile` puts every row on the per-tile
    build kernel, the walk's second instantiation in the engine."""
    for name in ("MR_COOC_LIGHT", "MR_COOC_GROUP"):
        monkeypatch.delenv(name, raising=False)
        if build == "pertile":
            monkeypatch.setenv(name, "0")
    with Engine(dataset(), out_dtype="f64", topk=10, frac_bits=32, stage1="wide", ibm_route="cooc",
                block_songs=TILE) as e:
        assert e.ibm_route == "cooc" and e.n_tiles == 2
        check_ibm(e)
