"""GPU: the top-k selection under adversarial structure (tests/topk_cases.py).

Random data keeps the threshold select's survivor count near k, so only one of
rank_survivors' three regimes runs, ties rarely straddle a tile or shard
boundary, and the candidate path's fp32 approximation never mis-orders the
songs at the k-th place. The cases here place the best songs of a tile by
hand. Every comparison is bitwise, songs and keys, against
oracle.native.fp_model, and every case re-asserts from the oracle's output
which regime its tile reaches before it compares: a case cannot silently run
another branch.
"""
import functools

import numpy as np
import pytest

import topk_cases as tc
from helpers import dataset_from_lines
from musicrecommendation_amd import _lib
from musicrecommendation_amd.engine import Engine, merge_topk_host
from musicrecommendation_amd.sharding import song_shards
from oracle import native

pytestmark = pytest.mark.gpu
MODELS = ("ibm", "ubm")
FUSED_CASES = [p for p in tc.PACKED if p.shape == "fused"]
WIDE_CASES = [p for p in tc.PACKED if p.shape == "wide"]


@functools.lru_cache(maxsize=None)
def dataset_of(kind, *args):
    case = {"packed": lambda p: tc.packed_case(p), "near": lambda k, f: tc.near_ties(k, frac_bits=f),
            "flood": tc.tie_flood, "boundary": tc.boundary_ties}[kind](*args)
    return case, dataset_from_lines(*case.lines)


@functools.lru_cache(maxsize=None)
def oracle_of(kind, args, model, k, frac_bits=32):
    """(dense, songs, keys) of the whole dataset, computed once and shared (read only)."""
    _, ds = dataset_of(kind, *args)
    out = native.fp_model(ds, model, k=k, frac_bits=frac_bits)
    for a in out:
        a.setflags(write=False)
    return out


def check_lists(ds, model, k, exp, *, dense=True, frac_bits=32, expect=None, **kw):
    """One engine run: songs, keys (and the dense scores) bitwise against the
    oracle's `exp`; `expect`: attributes the engine must report."""
    with Engine(ds, out_dtype="f64", topk=k, dense=dense, frac_bits=frac_bits, **kw) as e:
        for name, want in (expect or {}).items():
            assert getattr(e, name) == want, (name, getattr(e, name), want)
        e.run(model)
        songs, scores, keys = e.topk()
        got = e.dense() if dense else None
    d, ts, tk = exp
    assert np.array_equal(songs, ts), "top-k songs differ from the fixed-point oracle"
    assert np.array_equal(keys, tk), "top-k keys differ from the fixed-point oracle"
    valid = keys >= 0
    assert np.array_equal(scores[valid], keys[valid].view(np.float64)) and np.isnan(scores[~valid]).all()
    if dense:
        assert np.array_equal(got, d, equal_nan=True), "dense scores differ from the fixed-point oracle"


def assert_packed_regime(p, exp, ds):
    case, _ = dataset_of("packed", p)
    nc, regime = tc.tile_regime(tc.keys_of(exp[0][0]), case.info["blo"], min(case.info["bhi"], ds.n_songs),
                                tc.SHAPES[p.shape], p.k)
    assert (nc, regime) == (p.m + 1, p.regime)


# ---- fused and separate shapes: every regime, then the in-launch merge -------
@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("stage1", ["fused", "separate"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("p", FUSED_CASES, ids=lambda p: p.name)
def test_packed_rows_fused_separate(p, model, stage1, lists):
    """rank_survivors' parallel ranking (nc = k and 125..128: the unrolled
    loop's remainder), the one-wave select (129, 217, 256) and the overflow
    into block_topk (tiles of 1024 songs) and block_topk_wide (8192), in the
    middle one of three tiles; topk_lists=True takes the general path on the
    same data."""
    _, ds = dataset_of("packed", p)
    exp = oracle_of("packed", (p,), model, p.k)
    assert_packed_regime(p, exp, ds)
    check_lists(ds, model, p.k, exp, stage1=stage1, block_songs=p.block, topk_lists=lists,
                expect=dict(shape=stage1, block_songs=p.block, n_tiles=p.n_tiles))


# ---- wide shape, all-songs path ----------------------------------------------
@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("p", WIDE_CASES, ids=lambda p: p.name)
def test_packed_rows_wide(p, model, lists):
    """k_score_wide's threshold select (cap = min(256, 16 k)): k = 2 overflows
    at 33 survivors (one_wave cannot be reached: 32 < 129), k = 10 selects in
    one wave from 129 to 160 and overflows at 161, k = 16 up to 256."""
    _, ds = dataset_of("packed", p)
    exp = oracle_of("packed", (p,), model, p.k)
    assert_packed_regime(p, exp, ds)
    check_lists(ds, model, p.k, exp, stage1="wide", block_songs=p.block, topk_lists=lists,
                expect=dict(shape="wide", block_songs=p.block, n_tiles=p.n_tiles, candidate_topk=False))


# ---- wide shape, candidate path ------------------------------------------------
def cand_run(ds, model, k, exp, cand, monkeypatch, *, route="auto", frac_bits=32, **kw):
    """A top-k-only wide run of one tile, candidate path on or off."""
    monkeypatch.setenv("MR_WIDE_CAND", "1" if cand else "0")
    expect = dict(shape="wide", candidate_topk=cand, n_tiles=1)
    if route != "auto":
        expect["ibm_route"] = route
    check_lists(ds, model, k, exp, dense=False, stage1="wide", ibm_route=route, frac_bits=frac_bits,
                expect=expect, **kw)


@functools.lru_cache(maxsize=None)
def near_checked(k, frac_bits):
    """The near-tie dataset with its properties re-asserted from the oracle:
    each pair sits at places k and k + 1 of its user, and the candidate path's
    tau is one of the pair's approximations."""
    case, ds = dataset_of("near", k, frac_bits)
    _, ts, _ = oracle_of("near", (k, frac_bits), "ibm", k + 1, frac_bits)
    heard = ds.heard_mask()
    found = set()
    for fam in case.info["families"]:
        u, b, w = fam["user"], fam["better"], fam["worse"]
        assert ts[u, k - 1] == b and ts[u, k] == w
        acc = tc.accumulators(ds, "ibm", u, frac_bits)
        a = tc.approx_f32(acc, ds.song_count, True)
        nc, regime, tau = tc.cand_tile_regime(a, heard[u], 0, ds.n_songs, tc.SHAPES["wide"], k)
        assert tau == max(a[b], a[w]) and regime == "parallel"
        if fam["family"] == "invert":
            assert a[b] < a[w]
        found.add(fam["family"])
    assert found == set(tc.FAMILIES)
    return ds


@pytest.mark.parametrize("frac_bits", [32, 40])
@pytest.mark.parametrize("cand", [True, False])
@pytest.mark.parametrize("route", ["cooc", "two_hop"])
@pytest.mark.parametrize("k", [1, 4, 10, 16])
def test_near_ties_candidate_path(k, route, cand, frac_bits, monkeypatch):
    """ItemBasedModel scores from different (C, c) that are the same real number
    or within 2^-17 of each other, at the k-th place: fp32 approximations that
    order the other way or coincide must not lose the better song."""
    ds = near_checked(k, frac_bits)
    assert ds.n_songs <= 1024 * 20  # one tile
    exp = oracle_of("near", (k, frac_bits), "ibm", k, frac_bits)
    cand_run(ds, "ibm", k, exp, cand, monkeypatch, route=route, frac_bits=frac_bits)


@pytest.mark.parametrize("cand", [True, False])
@pytest.mark.parametrize("model,route", [("ibm", "cooc"), ("ibm", "two_hop"), ("ubm", "auto")])
@pytest.mark.parametrize("m", [140, 300])
def test_tie_flood_candidate_path(m, model, route, cand, monkeypatch):
    """m songs with one (accumulator, c) above the background, k = 10: tau > 0
    and every tied song survives the approximation's threshold, so 140 take the
    one-wave select and 300 overflow into the all-songs path."""
    case, ds = dataset_of("flood", m)
    exp = oracle_of("flood", (m,), model, 10)
    a = tc.approx_f32(tc.accumulators(ds, model, 0), ds.song_count, model == "ibm")
    nc, regime, tau = tc.cand_tile_regime(a, ds.heard_mask()[0], 0, ds.n_songs, tc.SHAPES["wide"], 10)
    assert tau > 0 and (nc, regime) == (m, "one_wave" if m == 140 else "overflow")
    cand_run(ds, model, 10, exp, cand, monkeypatch, route=route)


@pytest.mark.parametrize("cand", [True, False])
@pytest.mark.parametrize("m", [140, 300])
def test_tie_flood_cooc_512_threads(m, cand, monkeypatch):
    """The co-listening scoring kernel at 512 threads: cap = 80 lies below the
    parallel ranking's reach (90), so both floods overflow."""
    monkeypatch.setenv("MR_COOC_NT", "512")
    case, ds = dataset_of("flood", m)
    exp = oracle_of("flood", (m,), "ibm", 10)
    a = tc.approx_f32(tc.accumulators(ds, "ibm", 0), ds.song_count, True)
    nc, regime, tau = tc.cand_tile_regime(a, ds.heard_mask()[0], 0, ds.n_songs, tc.SHAPES["wide512"], 10)
    assert tau > 0 and (nc, regime) == (m, "overflow")
    cand_run(ds, "ibm", 10, exp, cand, monkeypatch, route="cooc", block_songs=8192)


# ---- ties astride tile and shard boundaries ---------------------------------------
def path_kwargs(path, monkeypatch):
    if path == "cand":
        monkeypatch.setenv("MR_WIDE_CAND", "1")
        return dict(dense=False, stage1="wide", expect=dict(shape="wide", candidate_topk=True))
    return dict(stage1=path, expect=dict(shape=path))


@pytest.mark.parametrize("path", ["fused", "separate", "wide", "cand"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", [1, 4, 10, 16])
def test_boundary_ties_three_tiles(k, model, path, monkeypatch):
    """Equal-score groups astride both boundaries of three 256-song tiles, the
    k-th place inside a group: the merge breaks the tie by song id across tiles."""
    case, ds = dataset_of("boundary", 256, 3)
    exp = oracle_of("boundary", (256, 3), model, k)
    assert exp[2][0, k - 1] == native.fp_model(ds, model, k=k + 1, dense=False)[2][0, k]  # the tie goes on past k
    kw = path_kwargs(path, monkeypatch)
    kw["expect"].update(block_songs=256, n_tiles=3)
    check_lists(ds, model, k, exp, block_songs=256, **kw)


@pytest.mark.parametrize("path", ["fused", "separate", "wide", "cand"])
@pytest.mark.parametrize("model", MODELS)
def test_boundary_ties_merge_beyond_registers(model, path, monkeypatch):
    """17 tiles x k = 16 = 272 candidates > 256: the in-launch merge stages the
    lists in LDS instead of holding one per thread (k_topk_merge in the wide shape)."""
    case, ds = dataset_of("boundary", 256, 17)
    exp = oracle_of("boundary", (256, 17), model, 16)
    kw = path_kwargs(path, monkeypatch)
    kw["expect"].update(block_songs=256, n_tiles=17)
    check_lists(ds, model, 16, exp, block_songs=256, **kw)


@pytest.mark.parametrize("stage1", ["fused", "separate"])
@pytest.mark.parametrize("model", MODELS)
def test_boundary_ties_multi_pass_merge(model, stage1):
    """45 tiles x k = 64: 42 lists fit one LDS pass, so the merge runs two, with
    the tie at the 64th place spread over eleven tile boundaries."""
    case, ds = dataset_of("boundary", 256, 45)
    exp = oracle_of("boundary", (256, 45), model, 64)
    check_lists(ds, model, 64, exp, stage1=stage1, block_songs=256, expect=dict(shape=stage1, n_tiles=45))


@pytest.mark.parametrize("stage1", ["fused", "wide"])
@pytest.mark.parametrize("model", MODELS)
def test_boundary_ties_song_shards(model, stage1):
    """Three song shards whose cuts fall inside tie groups, merged on the host
    and by the device merge kernel."""
    import torch

    k = 10
    case, ds = dataset_of("boundary", 256, 3)
    _, ts, tk = oracle_of("boundary", (256, 3), model, k)
    shards = song_shards(ds, 3)
    for lo, _hi in shards[1:]:
        assert any(a < lo < b for a, b, _ in case.info["groups"])
    ss, kk = [], []
    for lo, hi in shards:
        with Engine(ds, out_dtype="f64", topk=k, song_lo=lo, song_hi=hi, stage1=stage1, block_songs=256) as e:
            e.run(model)
            s, _, key = e.topk()
        _, os_, ok = native.fp_model(ds, model, song_lo=lo, song_hi=hi, k=k, dense=False)
        assert np.array_equal(s, os_) and np.array_equal(key, ok)
        ss.append(s)
        kk.append(key)
    ms, _msc, mk = merge_topk_host(np.stack(ss), np.stack(kk))
    assert np.array_equal(ms, ts) and np.array_equal(mk, tk)
    g_s = torch.tensor(np.stack(ss), device="cuda")
    g_k = torch.tensor(np.stack(kk), device="cuda")
    o_s, o_k = torch.empty_like(g_s[0]), torch.empty_like(g_k[0])
    o_sc = torch.empty(o_k.shape, dtype=torch.float64, device="cuda")
    with Engine(ds, topk=k) as e:
        e.merge_topk_device(3, g_s.data_ptr(), g_k.data_ptr(), o_s.data_ptr(), o_k.data_ptr(), o_sc.data_ptr())
    assert np.array_equal(o_s.cpu().numpy(), ts) and np.array_equal(o_k.cpu().numpy(), tk)


def test_device_merge_many_lists_multi_pass():
    """k_topk_merge over 200 lists of k = 16 (170 fit one LDS pass): the lists
    are the oracle's own top-k of 200 song ranges of the 17-tile boundary data,
    so tie groups straddle list boundaries in both passes."""
    import torch

    k, n_lists = 16, 200
    case, ds = dataset_of("boundary", 256, 17)
    _, ts, tk = oracle_of("boundary", (256, 17), "ibm", k)
    cuts = np.linspace(0, ds.n_songs, n_lists + 1).astype(int)
    parts = [native.fp_model(ds, "ibm", song_lo=int(a), song_hi=int(b), k=k, dense=False) for a, b in zip(cuts, cuts[1:])]
    g_s = torch.tensor(np.stack([p[1] for p in parts]), device="cuda")
    g_k = torch.tensor(np.stack([p[2] for p in parts]), device="cuda")
    o_s, o_k = torch.empty_like(g_s[0]), torch.empty_like(g_k[0])
    o_sc = torch.empty(o_k.shape, dtype=torch.float64, device="cuda")
    with Engine(ds, topk=k) as e:
        e.merge_topk_device(n_lists, g_s.data_ptr(), g_k.data_ptr(), o_s.data_ptr(), o_k.data_ptr(), o_sc.data_ptr())
    assert np.array_equal(o_s.cpu().numpy(), ts) and np.array_equal(o_k.cpu().numpy(), tk)
    assert np.array_equal(o_sc.cpu().numpy(), tk.view(np.float64))


# ---- k_topk_dense ------------------------------------------------------------------------
def dense_dataset():
    """5 test users x 2,301 songs (more than two songs per thread of k_topk_dense)."""
    n = 2300
    train = [f"t\t{tc.song(s)}\t1" for s in range(n)] + [f"t\t{tc.ANCHOR}\t1"]
    test = [f"x{u}\t{tc.ANCHOR}\t1" for u in range(5)]
    return dataset_from_lines(train, test, [f"x0\t{tc.song(0)}\t1"])


def numpy_topk(x, k):
    """(songs, keys) by (score desc, song asc); NaN = no pair; -0.0 has +0.0's key."""
    songs = np.full((x.shape[0], k), -1, dtype=np.int32)
    keys = np.full((x.shape[0], k), -1, dtype=np.int64)
    for u, row in enumerate(x.astype(np.float64)):
        valid = np.flatnonzero(~np.isnan(row))
        key = (row[valid] + 0.0).view(np.int64)
        order = np.lexsort((valid, -key))[:k]
        songs[u, :order.size] = valid[order]
        keys[u, :order.size] = key[order]
    return songs, keys


@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_topk_dense_ties_zero_nan(dtype, k):
    """A hand-built dense model: tie groups astride the threads' strides, -0.0
    and +0.0 (one key), an all-NaN row, rows with fewer than k valid entries,
    then a model with one negative score (MR_E_INVALID, and no list to read),
    then the valid model again."""
    import torch

    from musicrecommendation_amd.ensemble import DeviceEnsemble

    ds = dense_dataset()
    npt = np.float32 if dtype == "f32" else np.float64
    rng = np.random.default_rng(3)
    x = np.full((ds.n_test, ds.n_songs), np.nan, dtype=npt)
    x[0] = rng.integers(0, 40, ds.n_songs).astype(npt) / 8          # heavy ties everywhere
    x[0, [7, 1031, 2055, 1030, 6]] = 9.5                              # a tie over one thread's songs and its neighbours
    x[1, 3::5] = 0.0                                                  # zeros of both signs only
    x[1, 8::10] = -0.0
    x[2] = np.nan                                                     # no pair at all
    x[3, [2299, 5, 1024]] = [0.25, 0.25, -0.0]                        # 3 valid entries
    x[4] = rng.random(ds.n_songs).astype(npt)
    x[4, 100:140] = x[4].max()                                        # 40 equal maxima
    x[4, ::3] = np.nan
    exp_s, exp_k = numpy_topk(x, k)
    assert (exp_s[2] == -1).all() and (exp_s[3, 3:] == -1).all() and (exp_k[1][exp_s[1] >= 0] == 0).all()
    bad = x.copy()
    bad[4, 1500] = -1e-3
    with Engine(ds, out_dtype=dtype, topk=k) as e:
        ens = DeviceEnsemble(e)
        good_t, bad_t = (torch.tensor(a, device="cuda") for a in (x, bad))

        def valid_call():
            songs, scores, keys = ens.topk(good_t)
            assert np.array_equal(songs, exp_s) and np.array_equal(keys, exp_k)
            ok = keys >= 0
            assert np.array_equal(scores[ok], keys[ok].view(np.float64)) and np.isnan(scores[~ok]).all()

        valid_call()
        with pytest.raises(_lib.EngineError) as ei:
            ens.topk(bad_t)
        assert ei.value.code == _lib.MR_E_INVALID
        with pytest.raises(_lib.EngineError):  # the lists that skip the negative score are not output
            e.topk()
        valid_call()
