"""The builders of tests/cooc_limit_cases.py deliver the counts they state
(no GPU): exact C[hub][twin] and graded counts from a set-based numpy count,
the adjacent tile-local ids, the dense rule on the tiles named, the light-row
bound of the 4095 hub, the split-sum window past 2^31, and the fixed-point
oracle itself against a direct integer restatement at 17-bit counts."""
import re
from pathlib import Path

import numpy as np
import pytest

import cooc_limit_cases as cl
from oracle import native

SRC = (Path(__file__).resolve().parents[1] / "musicrecommendation_amd" / "csrc" / "mr_engine.hip").read_text()


@pytest.fixture(scope="module")
def nested():
    return cl.nested_hubs()


@pytest.fixture(scope="module")
def split():
    return cl.split_sum_users()


def test_constants_match_the_source():
    """The limits this module states are those of csrc/mr_engine.hip."""
    def const(name):
        m = re.search(r"constexpr \w+ " + name + r" = ([^;]+);", SRC)
        assert m, name
        return m.group(1).strip()

    assert const("kLightCntBits") == "12" and cl.LIGHT_CNT_MAX == (1 << 12) - 1
    assert const("kCoocCntBits") == "17" and cl.CNT_MAX == (1 << 17) - 1
    assert const("kLightSlots") == "32768"
    assert const("kLightMaxTiles") == str(cl.LIGHT_MAX_TILES)
    assert const("kLightMaxWidth") == "(1 << (32 - kLightCntBits)) - 2"
    assert const("kWaveMaxTiles") == str(cl.WAVE_MAX_TILES)
    assert const("kMaxGroupTiles") == str(cl.NARROW_TILES)
    assert const("kCoocDenseDiv") == str(cl.DENSE_DIV)
    assert "p.all32 || listeners >= 65536" in SRC
    assert "c <= (int32_t)kLightCntMask" in SRC and "p.row_base[r] * 100 <= light_slots_max * lload" in SRC
    assert "p.urec_words <= 32 && p.max_shard_deg <= 65535" in SRC
    assert "std::min(std::min(p.cooc_nt, (WL.total - WL.wk - 8) / 40), 255)" in SRC
    assert 1 + (cl.GROUP_MAX_TILES + 2) // 2 == 32 and 1 + (cl.GROUP_MAX_TILES + 3) // 2 == 33


def test_nested_hubs_counts(nested):
    ds, S, info = nested.ds, nested.songs, nested.info
    assert ds.n_train == 131071 and ds.n_test == 12 and ds.n_songs == info["n_songs"]
    assert int(ds.tr_off[-1]) + int(ds.te_off[-1]) < 1_500_000
    c_tr = np.bincount(ds.tr_songs, minlength=ds.n_songs)
    for n in info["sizes"]:
        hub, twin = S[f"hub{n}"], S[f"twin{n}"]
        assert np.array_equal(cl.listeners(ds, hub), np.arange(n))       # the nested sets
        assert np.array_equal(cl.listeners(ds, twin), np.arange(n))
        C = cl.cooc_row(ds, hub)
        assert C[twin] == n and C[hub] == n
        # every hub and twin column: the smaller listener set
        for m in info["sizes"]:
            assert C[S[f"hub{m}"]] == min(n, m) and C[S[f"twin{m}"]] == min(n, m)
        # the 65535 twins and their word neighbours (u16 pairs: songs 2w, 2w + 1 of a tile)
        assert (C[4], C[5]) == (min(n, 65535),) * 2
        assert (C[6], C[7]) == (min(n, 65535), 1) and (C[8], C[9]) == (1, min(n, 65535))
        # the graded tile: min(g, n), all 256 non-zero, so dense under nnz * 3 >= songs
        g = info["graded"]
        assert np.array_equal(C[256:512], np.minimum(g, n))
        assert (C[256:512] > 0).sum() * cl.DENSE_DIV >= 256
        if n >= 65535:
            assert {1, 2, 255, 256, 4095 - 255, 65535 - 255} <= set((C[256:512] - 255).tolist())
    for v in cl.GRADED_SPECIAL + (131071,):
        assert v in info["graded"][:14]
    assert set(cl.cooc_row(ds, S["hub_top"])[256:512] - 255) >= {1, 2, 255, 256, 130816}
    assert c_tr[S["hub_top"]] == cl.CNT_MAX and c_tr[S["hub65535"]] == 0xffff and c_tr[S["hub4095"]] == cl.LIGHT_CNT_MAX
    # adjacent tile-local ids in one u16-pair word
    for even in (4, 6, 8):
        assert even % 2 == 0 and even // 256 == (even + 1) // 256
    # every row length mod 8 among the first users (the light rows' 16-B chunks)
    assert set((np.diff(ds.tr_off)[:4095] % 8).tolist()) == set(range(8))
    assert c_tr[S["cold"]] == 0 and S["cold"] == ds.n_songs - 1


@pytest.mark.parametrize("block", sorted(cl.NESTED_CUTS))
def test_nested_hubs_index_kinds(nested, block):
    """Under mr_load's rules the cut shards hold light, u16 and u32 rows; the
    4095 hub is light (its bound fits the largest table) and the 4096 hub is not."""
    ds, S = nested.ds, nested.songs
    hi = cl.NESTED_CUTS[block]
    m = cl.index_model(ds, 0, hi, block)
    kind = dict(zip(m["rows"].tolist(), m["kind"].tolist()))
    bound = dict(zip(m["rows"].tolist(), m["bound"].tolist()))
    assert cl.NARROW_TILES < m["n_tiles"] <= cl.GROUP_MAX_TILES and m["max_deg"] <= cl.GROUP_MAX_DEG
    assert bound[S["hub4095"]] * 100 <= 32768 * 80
    assert kind[S["hub4095"]] == "light" and kind[S["hub4096"]] == "u16"
    assert kind[S["hub65535"]] == "u16" and kind[S["twin65535"]] == "u16"
    assert kind[S["hub65536"]] == "u32" and kind[S["hub_top"]] == "u32"
    assert {"light", "u16", "u32"} == set(m["kind"].tolist())
    assert m["dense_songs"] > 0
    if block == 256:
        assert {1, 2, 255, 256, 130816} <= set(m["excess"])


def test_nested_hubs_131072():
    for heard in (True, False):
        case = cl.nested_hubs(top=131072, top_heard=heard)
        ds = case.ds
        c_tr = np.bincount(ds.tr_songs, minlength=ds.n_songs)
        assert ds.n_train == 131072 and c_tr[case.songs["hub_top"]] == 131072 > cl.CNT_MAX
        assert c_tr.max() == 131072
        rows = np.unique(ds.te_songs)
        assert (c_tr[rows].max() == 131072) == heard
        if not heard:  # a column only: every count is at most its row's listeners
            assert c_tr[rows].max() == 65536
            assert cl.cooc_row(ds, case.songs["hub65536"])[case.songs["hub_top"]] == 65536


def test_oracle_restated_at_17_bit_counts(nested):
    """native.fp_model on the hub rows equals acc[s] = Σ_{s2 ∈ T(u)} q(s2) C[s2][s],
    score = (acc 2^-32) / sqrt c(s), in exact integers."""
    ds = nested.ds
    got, _, _ = native.fp_model(ds, "ibm", k=1)
    q = cl.q32(ds.song_count)
    sqrt_c = np.sqrt(ds.song_count.astype(np.float64))
    user_of = cl.train_user_of_entry(ds)
    for u in (nested.users[x] for x in ("hub4095", "hub65535", "hub_top", "all_hubs", "top_graded", "twin_only")):
        mine = ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]]
        acc = np.zeros(ds.n_songs, np.int64)
        for s2 in mine.tolist():
            acc += int(q[s2]) * cl.cooc_row(ds, s2, user_of)
        assert acc.max() < 2 ** 62
        exp = (acc.astype(np.float64) * 2.0 ** -32) / sqrt_c
        exp[mine] = np.nan
        assert np.array_equal(got[u], exp, equal_nan=True), f"test user {u}"


def test_split_sum_window(split):
    ds, info = split.ds, split.info
    c = info["counts"]
    assert c.size >= 300 and c.min() >= 255 and c.max() <= 3000
    assert ((cl.q32(c) & 0xffff) >= 0xC000).all()
    assert np.array_equal(ds.song_count[info["ids"]], c)
    assert (ds.song_count[list(cl.SPLIT_SINGLES)] == 2).all()
    assert {s % 2 for s in cl.SPLIT_SINGLES} == {0, 1}
    assert -(-ds.n_songs // cl.SPLIT_BLOCK) > cl.LIGHT_MAX_TILES    # no light rows: every row heavy
    # rows per descriptor pass: the wide shape keeps topk <= 16, so 133 is the most (255 would take topk = 40)
    assert [cl.split_nseg(k) for k in (1, 10, 16)] == [57, 102, 133] and cl.split_nseg(16, nt=512) == 81
    assert cl.split_nseg(39) < 255 == cl.split_nseg(40) and re.search(r"kMaxTopkLarge = 16;", SRC)
    nseg = cl.split_nseg(cl.SPLIT_K)
    assert cl.SPLIT_K == 16 and nseg == cl.SPLIT_PEAK == 133
    assert ds.te_off[1] > 2 * nseg and ds.te_off[2] - ds.te_off[1] == 255
    # test user 1's first pass: exactly the SPLIT_PEAK rows of the largest q & 0xffff
    first = ds.te_songs[ds.te_off[1]:ds.te_off[1] + nseg]
    assert np.array_equal(first, info["ids"][:nseg])
    low = cl.q32(ds.song_count[info["ids"]]) & 0xffff
    assert low[:nseg].min() >= low[nseg:].max() and low.min() >= 0xC000
    a = split.songs["tile_lo"]
    user_of = cl.train_user_of_entry(ds)
    for s2 in list(cl.SPLIT_SINGLES) + info["ids"][[0, 150, 299]].tolist():
        C = cl.cooc_row(ds, s2, user_of)[a:a + 256]
        assert (C > 0).sum() >= 86 and (C > 0).sum() * cl.DENSE_DIV >= 256          # dense in the tile
        assert (C >= 255).all() if s2 not in cl.SPLIT_SINGLES else (C == 1).all()    # saturated bytes
    lo, hi = cl.split_sum_window(ds, nseg)
    print(f"split-sum window at nseg = {nseg}: max lo = {lo} ({lo / 2 ** 32:.4f} x 2^32), max hi = {hi}")
    assert 2 ** 31 <= lo < 2 ** 32 and hi < 2 ** 32


@pytest.mark.parametrize("n", [65535, 65536])
def test_whale(n):
    case = cl.whale(n)
    ds = case.ds
    assert np.diff(ds.tr_off).max() == n == ds.n_songs
    m = cl.index_model(ds, 0, ds.n_songs, cl.WHALE_BLOCK)
    assert m["max_deg"] == n and cl.NARROW_TILES < m["n_tiles"] <= cl.GROUP_MAX_TILES
    assert (m["listeners"] == cl.WHALE_OTHERS + 1).all() and (m["kind"] == "u16").all()
    assert (m["bound"] == ds.n_songs).all()   # min(width, Σ deg) = width
    for h in cl.WHALE_HUBS:
        assert (cl.cooc_row(ds, h)[:n] > 0).all()


def test_tile_cuts():
    case = cl.tile_cuts()
    ds = case.ds
    assert ds.n_songs == cl.CUT_SONGS >= 65792
    assert max(len(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]]) for u in range(ds.n_test)) <= 8
    for t in cl.CUT_TILES:
        m = cl.index_model(ds, 0, 256 * t, cl.CUT_BLOCK)
        kinds = set(m["kind"].tolist())
        assert ("light" in kinds) == (t <= cl.LIGHT_MAX_TILES) and "u16" in kinds
        assert m["dense_songs"] > 0 and m["max_deg"] <= cl.GROUP_MAX_DEG
    # every tile has a non-zero in the dense hub's row; the sparse hub's row stays sparse somewhere
    C = cl.cooc_row(ds, case.songs["dense_hub"])
    assert ((C[:256 * 257].reshape(257, 256) > 0).sum(axis=1) * cl.DENSE_DIV >= 256).all()
    C = cl.cooc_row(ds, case.songs["sparse_hub"])
    nz = (C[:256 * 257].reshape(257, 256) > 0).sum(axis=1)
    assert (nz > 0).all() and (nz * cl.DENSE_DIV < 256).any()
