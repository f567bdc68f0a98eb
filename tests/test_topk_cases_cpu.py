"""The adversarial top-k generators (tests/topk_cases.py) against the CPU
oracle: every generated tile lands in the regime its case names, the near-tie
data really holds the inversions it is built for, and the flood and boundary
cases have the stated tie counts. No GPU."""
import os
import re

import numpy as np
import pytest

import topk_cases as tc
from helpers import dataset_from_lines
from musicrecommendation_amd.sharding import song_shards
from oracle import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("ibm", "ubm")


def oracle_keys(ds, model, k, user, frac_bits=32):
    dense, ts, tk = native.fp_model(ds, model, k=k, frac_bits=frac_bits, user_lo=user, user_hi=user + 1)
    return tc.keys_of(dense[0]), ts[0], tk[0]


def test_constants_match_the_kernel_source():
    with open(os.path.join(ROOT, "musicrecommendation_amd", "csrc", "mr_engine.hip")) as f:
        src = f.read()

    def const(pattern):
        m = re.search(pattern, src)
        assert m, pattern
        return int(m.group(1))

    f, w = tc.SHAPES["fused"], tc.SHAPES["wide"]
    assert const(r"constexpr int kThreads = (\d+);") == f.nt == tc.SHAPES["separate"].nt
    assert const(r"#define MR_TILE_ROWS (\d+)") == f.ng
    assert const(r"#define MR_RANK_Q_FUSED (\d+)") == f.rank_q
    assert const(r"constexpr int kWideThreads = (\d+);") == w.nt
    assert const(r"#define MR_RANK_Q_WIDE (\d+)") == w.rank_q == tc.SHAPES["wide512"].rank_q
    assert (f.nt // 64) * const(r"constexpr int kMaxTopK = (\d+);") == tc.cap_of(f, 10) == 256
    assert "template <int NT, typename Get, int NG = NT / 16>" in src  # the wide kernels' rows
    for s in (w, tc.SHAPES["wide512"]):
        assert s.ng == s.nt // 16 and s.lists == s.nt // 64
    assert "min(256, NW * k)" in src and "nc * nc > kRankQ<NT> * NT" in src
    assert "(1.f - 0x1p-17f)" in src
    # the parallel ranking's reach: nc <= 128 in the 256- and 1024-thread kernels, 90 at 512
    assert [max(n for n in range(1, 257) if n * n <= s.rank_q * s.nt) for s in (f, w, tc.SHAPES["wide512"])] == \
        [128, 128, 90]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("p", tc.PACKED, ids=lambda p: p.name)
def test_packed_rows_reach_their_regime(p, model):
    case = tc.packed_case(p)
    ds = dataset_from_lines(*case.lines)
    info = case.info
    assert ds.n_songs == info["n_songs"] and ds.song_names(info["pivot"]) == tc.song(info["pivot"])
    keys, ts, _ = oracle_keys(ds, model, p.k, 0)
    shape = tc.SHAPES[p.shape]
    assert -(-ds.n_songs // p.block) == p.n_tiles
    nc, regime = tc.tile_regime(keys, info["blo"], min(info["bhi"], ds.n_songs), shape, p.k)
    assert (nc, regime) == (p.m + 1, p.regime)
    # the m packed songs are the tile's best, above the pivot, above a positive background
    tile = keys[info["blo"]:info["bhi"]]
    packed = keys[info["packed"]]
    rest = np.setdiff1d(np.arange(info["blo"], info["bhi"]), info["packed"] + [info["pivot"]])
    rest = rest[keys[rest] >= 0]
    assert packed.min() > keys[info["pivot"]] > keys[rest].max() and keys[rest].min() > 0
    assert np.unique(packed).size == (1 if p.tied else p.m)
    assert (tile >= 0).sum() == tile.size - (1 if info["bhi"] >= ds.n_songs else 0)  # only the anchor is heard
    # the merged list draws from the other tiles too (ties in tile 0 fill it with tile 0's lowest ids)
    if p.m >= 2 and not (p.tied and p.tile == 0):
        assert len({int(s) // p.block for s in ts if s >= 0}) >= 2


def test_packed_cases_cover_every_reachable_regime():
    seen = {(p.shape, p.k, p.regime) for p in tc.PACKED}
    for shape in ("fused", "wide"):
        assert {r for s, _, r in seen if s == shape} == {"parallel", "one_wave", "overflow"}
    # the unrolled comparison loop's remainder: survivor counts that are no multiple of 4
    ncs = [p.m + 1 for p in tc.PACKED if p.shape == "fused" and p.regime == "parallel"]
    assert sum(1 for n in ncs if n % 4) >= 2 and {10, 125, 126, 127, 128} <= set(ncs)
    # wide, k = 2: cap = 32 < 129, so one_wave cannot be reached; k = 10 and 16 reach all three
    assert tc.cap_of(tc.SHAPES["wide"], 2) == 32
    assert ("wide", 2, "one_wave") not in seen and ("wide", 2, "overflow") in seen
    for k in (10, 16):
        assert {r for s, kk, r in seen if s == "wide" and kk == k} >= {"one_wave", "overflow"}
    # overflow fall-backs: block_topk (tiles <= 1024 songs) and block_topk_wide
    assert {p.block <= 1024 for p in tc.PACKED if p.shape == "fused" and p.regime == "overflow"} == {True, False}


@pytest.mark.parametrize("frac_bits", [32, 40])
def test_near_tie_pairs_families(frac_bits):
    pairs = tc.near_tie_pairs(frac_bits)
    q = int(np.rint(2.0 ** frac_bits / np.sqrt(tc.NEAR_A + 1.0)))

    def both(p):
        acc, c = np.array([p[0] * q]), np.array([p[1]])
        return tc.exact_scores(acc, c, True, frac_bits).view(np.int64)[0], tc.approx_f32(acc, c, True)[0]

    for name in tc.FAMILIES:
        assert pairs[name], f"no {name} pair found"
    for p, r in pairs["invert"]:
        (kp, ap), (kr, ar) = both(p), both(r)
        assert kp > kr and ap < ar and ap >= ar * tc.CAND_MARGIN  # the margin absorbs the inversion
    for p, r in pairs["equal_approx"]:
        (kp, ap), (kr, ar) = both(p), both(r)
        assert kp > kr and ap == ar
    for p, r in pairs["equal_key"]:
        (kp, ap), (kr, ar) = both(p), both(r)
        assert p != r and kp == kr and p[0] ** 2 * r[1] == r[0] ** 2 * p[1]  # the same real number
        assert ap <= ar
    for p, r in pairs["int_near"]:
        (kp, _), (kr, _) = both(p), both(r)
        sp, sr = (np.array([x], dtype=np.int64).view(np.float64)[0] for x in (kp, kr))
        assert abs(p[0] ** 2 * r[1] - r[0] ** 2 * p[1]) == 1 and 0 < (sp - sr) / sr < 2.0 ** -17
    for p, r in pairs["control"]:
        (kp, ap), (kr, ar) = both(p), both(r)
        sp, sr = (np.array([x], dtype=np.int64).view(np.float64)[0] for x in (kp, kr))
        assert 2.0 ** -17 < (sp - sr) / sr < 2.0 ** -15 and ap > ar


@pytest.mark.parametrize("frac_bits", [32, 40])
@pytest.mark.parametrize("k", [1, 4, 10, 16])
def test_near_ties_sit_at_the_kth_place(k, frac_bits):
    case = tc.near_ties(k, frac_bits=frac_bits)
    ds = dataset_from_lines(*case.lines)
    assert ds.n_songs == case.info["n_songs"]
    heard = ds.heard_mask()
    seen = set()
    for fam in case.info["families"]:
        u, b, w = fam["user"], fam["better"], fam["worse"]
        assert ds.test_names(u) == f"x{u:02d}"
        keys, ts, _ = oracle_keys(ds, "ibm", k + 1, u, frac_bits)
        # places 1 .. k-1: the strong songs; k: the better member; k + 1: the other
        assert sorted(ts[:k - 1].tolist()) == fam["strong"] and ts[k - 1] == b and ts[k] == w
        acc = tc.accumulators(ds, "ibm", u, frac_bits)
        assert np.array_equal(tc.keys_of(np.where(heard[u], np.nan, tc.exact_scores(acc, ds.song_count, True, frac_bits))),
                              keys), "the accumulator model differs from the oracle"
        a = tc.approx_f32(acc, ds.song_count, True)
        name = fam["family"]
        if name == "invert":
            assert keys[b] > keys[w] and a[b] < a[w]
        elif name == "equal_approx":
            assert keys[b] > keys[w] and a[b] == a[w]
        elif name == "equal_key":
            assert keys[b] == keys[w] and b < w and fam["pair"][0] != fam["pair"][1]
        elif name == "int_near":
            sb, sw = (np.array([keys[x]]).view(np.float64)[0] for x in (b, w))
            assert 0 < (sb - sw) / sw < 2.0 ** -17
        else:
            sb, sw = (np.array([keys[x]]).view(np.float64)[0] for x in (b, w))
            assert (sb - sw) / sw > 2.0 ** -17
        # one tile, the candidate path: tau itself is one of the pair, and a handful survive
        nc, regime, tau = tc.cand_tile_regime(a, heard[u], 0, ds.n_songs, tc.SHAPES["wide"], k)
        assert tau == max(a[b], a[w]) and regime == "parallel" and k <= nc <= k + 1
        seen.add(name)
    assert seen == set(tc.FAMILIES)


@pytest.mark.parametrize("m", [140, 300])
def test_tie_flood_counts_and_regimes(m):
    case = tc.tie_flood(m)
    ds = dataset_from_lines(*case.lines)
    heard = ds.heard_mask()
    for model in MODELS:
        keys, ts, _ = oracle_keys(ds, model, 10, 0)
        flood = keys[case.info["flood"]]
        assert np.unique(flood).size == 1 and (keys == flood[0]).sum() == m and (keys > flood[0]).sum() == 0
        rest = keys[(keys >= 0) & (keys != flood[0])]
        assert 0 < rest.min() and rest.max() < flood[0]
        assert ts.tolist() == case.info["flood"][:10]
        acc = tc.accumulators(ds, model, 0)
        assert np.unique(acc[case.info["flood"]]).size == 1 and np.unique(ds.song_count[case.info["flood"]]).size == 1
        a = tc.approx_f32(acc, ds.song_count, model == "ibm")
        # the approximation's threshold keeps every tied song: tau > 0, nc = m
        nc, regime, tau = tc.cand_tile_regime(a, heard[0], 0, ds.n_songs, tc.SHAPES["wide"], 10)
        assert tau > 0 and nc == m and regime == ("one_wave" if m == 140 else "overflow")
        # 512 threads: cap = 80 is below the parallel reach of 90, one_wave cannot be reached
        nc, regime, _ = tc.cand_tile_regime(a, heard[0], 0, ds.n_songs, tc.SHAPES["wide512"], 10)
        assert nc == m and regime == "overflow"


@pytest.mark.parametrize("block,n_tiles,ks", [(256, 3, (1, 4, 10, 16)), (256, 17, (16,)), (256, 45, (64,))])
def test_boundary_ties_groups(block, n_tiles, ks):
    case = tc.boundary_ties(block, n_tiles)
    ds = dataset_from_lines(*case.lines)
    assert ds.n_songs == case.info["n_songs"] and -(-ds.n_songs // block) == n_tiles
    groups = case.info["groups"]
    for t in range(1, n_tiles):  # a group astride every tile boundary
        assert any(lo < t * block < hi for lo, hi, _ in groups)
    cuts = [lo for lo, _ in song_shards(ds, case.info["n_shards"])[1:]]
    for cut in cuts:  # and astride every shard cut
        assert any(lo < cut < hi for lo, hi, _ in groups), (cut, groups)
    for model in MODELS:
        keys, ts, tk = oracle_keys(ds, model, max(ks) + 1, 0)
        for lo, hi, lvl in groups:
            assert np.unique(keys[lo:hi]).size == 1
            same = sum(h - l for l, h, v in groups if v == lvl)
            assert (keys == keys[lo]).sum() == same  # the stated tie count of the level
        for k in ks:  # the k-th place falls inside a group: the (k + 1)-th song has the same key
            assert tk[k - 1] == tk[k] and ts[k - 1] < ts[k], k
            assert any(lo <= ts[k - 1] and ts[k] < hi for lo, hi, _ in groups) or ts[k] - ts[k - 1] > 1
        assert len({int(s) // block for s in ts}) >= 2
