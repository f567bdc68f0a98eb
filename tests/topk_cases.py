"""Adversarial top-k inputs and a model of which selection branch they reach.

Plain helper module (no tests). The selection code of csrc/mr_engine.hip picks
its branch from the data: block_topk_threshold takes tau = the k-th best of the
NG row bests, collects every entry at or before tau (nc survivors) and
rank_survivors then ranks them in parallel, hands them to one wave, or reports
an overflow that sends the caller to a per-thread-list path. Random data keeps
nc near k, so the generators here place the best songs of a tile by hand.

The numpy models below CLASSIFY inputs only (which regime a tile reaches, which
songs the candidate path's fp32 approximation would mis-order). Expected
outputs always come from oracle.native.fp_model.

Constants, from csrc/mr_engine.hip (tests/test_topk_cases_cpu.py re-reads them
from the source so that a change there is noticed):
  kThreads = 256 (:59), kMaxTopK = 64 (:61), MR_TILE_ROWS = 32 (:49): the fused
    and separate shapes' k_score calls block_topk_threshold<256, ., 32> with
    cap = kWaves * kMaxTopK = 256 (:1526-1527);
  kWideThreads = 1024 (:1754), NG = NT / 16 (:781, :1972): k_score_wide calls
    block_topk_threshold<NT> / wide_cand_topk with cap = min(256, NW * k),
    NW = NT / 64 (:2452-2453, :2537-2538); NT = 512 with MR_COOC_NT=512 on the
    co-listening route (:4150-4153);
  MR_RANK_Q_FUSED = 64 (:635), MR_RANK_Q_WIDE = 16 (:638): rank_survivors ranks
    in parallel while nc * nc <= kRankQ<NT> * NT (:659), i.e. nc <= 128 at
    NT = 256 and 1024, nc <= 90 at NT = 512;
  the candidate margin 1 - 2^-17 (:2020).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

INT_MAX = 2 ** 31 - 1
KEY_NONE = -1


class Shape(NamedTuple):
    nt: int                 # threads per workgroup
    ng: int                 # threshold rows (NT / NG consecutive threads each)
    rank_q: int             # kRankQ<NT>
    lists: Optional[int]    # cap = min(256, lists * k); None: cap = 256


SHAPES = {
    "fused": Shape(256, 32, 64, None),
    "separate": Shape(256, 32, 64, None),
    "wide": Shape(1024, 64, 16, 16),
    "wide512": Shape(512, 32, 16, 8),
}
CAND_MARGIN = np.float32(1.0) - np.float32(2.0 ** -17)


def cap_of(shape: Shape, k: int) -> int:
    return 256 if shape.lists is None else min(256, shape.lists * k)


# ---------------------------------------------------------------------------
# regime model
# ---------------------------------------------------------------------------
def keys_of(dense_row: np.ndarray) -> np.ndarray:
    """The engine's int64 keys of one dense f64 row: the score's bit pattern, -1 for NaN."""
    row = np.ascontiguousarray(dense_row, dtype=np.float64)
    return np.where(np.isnan(row), KEY_NONE, row.view(np.int64))


def block_tau(keys: np.ndarray, songs: np.ndarray, nt: int, ng: int, k: int) -> Tuple[int, int]:
    """block_tau: the k-th best (key desc, song asc) of the NG row bests; thread
    i % nt owns tile-local index i, a row is nt / ng consecutive threads.
    (0, INT_MAX) = "every valid key" when fewer than k rows hold an entry."""
    gs = nt // ng
    row = (np.arange(keys.shape[0]) % nt) // gs
    bests = []
    for r in np.unique(row[keys >= 0]):
        sel = np.flatnonzero((row == r) & (keys >= 0))
        j = sel[np.lexsort((songs[sel], -keys[sel]))[0]]
        bests.append((int(keys[j]), int(songs[j])))
    if len(bests) < k:
        return 0, INT_MAX
    bests.sort(key=lambda t: (-t[0], t[1]))
    return bests[k - 1]


def regime_of(nc: int, shape: Shape, k: int) -> str:
    if k > shape.ng or nc > cap_of(shape, k):
        return "overflow"
    return "one_wave" if nc * nc > shape.rank_q * shape.nt else "parallel"


def tile_regime(keys_row: np.ndarray, blo: int, bhi: int, shape: Shape, k: int) -> Tuple[int, str]:
    """(nc, regime) of block_topk_threshold on the tile [blo, bhi) of one user's
    keys (indexed by global song id)."""
    keys = np.asarray(keys_row[blo:bhi], dtype=np.int64)
    songs = np.arange(blo, bhi)
    tk, ts = block_tau(keys, songs, shape.nt, shape.ng, k)
    surv = (keys >= 0) & ((keys > tk) | ((keys == tk) & (songs <= ts)))
    nc = int(surv.sum())
    return nc, regime_of(nc, shape, k)


# ---------------------------------------------------------------------------
# the candidate path's fp32 approximation (wide_cand_topk)
# ---------------------------------------------------------------------------
def accumulators(ds, model: str, u: int, frac_bits: int = 32) -> np.ndarray:
    """The int64 fixed-point accumulator of every song for test user u (the
    sums of oracle/fixedpoint.c, as dense numpy products; small datasets)."""
    m = np.zeros((ds.n_train, ds.n_songs), dtype=np.int64)
    m[np.repeat(np.arange(ds.n_train), np.diff(ds.tr_off)), ds.tr_songs] = 1
    t = np.asarray(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]])
    two_f = 2.0 ** frac_bits
    if model == "ibm":
        q = np.rint(two_f / np.sqrt(ds.song_count.astype(np.float64))).astype(np.int64)
        qv = m[:, t] @ q[t]
    else:
        y = m[:, t].sum(axis=1)
        c = y.astype(np.float64) / (np.sqrt(float(ds.te_len[u])) * np.sqrt(ds.tr_len.astype(np.float64)))
        qv = np.where(y > 0, np.rint(c * two_f), 0.0).astype(np.int64)
    return qv @ m


def exact_scores(acc: np.ndarray, count: np.ndarray, ibm: bool, frac_bits: int = 32) -> np.ndarray:
    """The epilogue's fp64 operations (the oracle's): (acc * 2^-F) / sqrt(c)."""
    s = acc.astype(np.float64) * 2.0 ** -frac_bits
    return s / np.sqrt(count.astype(np.float64)) if ibm else s


def approx_f32(acc: np.ndarray, count: np.ndarray, ibm: bool) -> np.ndarray:
    """wide_cand_topk's approximation: fma(float(hi32), 2^32, float(lo32)) times
    the fp32 table entry float(1 / sqrt(double(c))) (1 for ubm). The fma's sum
    is formed exactly in fp64 here, which needs acc < 2^53."""
    acc = np.asarray(acc, dtype=np.int64)
    assert acc.min() >= 0 and acc.max() < 2 ** 53
    hi = (acc >> 32).astype(np.float32)
    lo = (acc & 0xFFFFFFFF).astype(np.float32)
    v = (hi.astype(np.float64) * 4294967296.0 + lo.astype(np.float64)).astype(np.float32)
    if not ibm:
        return v
    rv = (1.0 / np.sqrt(np.asarray(count, dtype=np.float64))).astype(np.float32)
    return v * rv


def cand_tile_regime(approx: np.ndarray, heard: np.ndarray, blo: int, bhi: int, shape: Shape,
                     k: int) -> Tuple[int, str, float]:
    """(nc, regime, tau) of wide_cand_topk on the tile [blo, bhi): tau = the k-th
    best row best of the approximations, survivors a >= tau * (1 - 2^-17)."""
    a = np.where(heard[blo:bhi], np.float32(-1), approx[blo:bhi]).astype(np.float32)
    songs = np.arange(blo, bhi)
    akey = np.where(a >= 0, a.view(np.uint32).astype(np.int64), KEY_NONE)
    tk, _ = block_tau(akey, songs, shape.nt, shape.ng, k)
    tau = np.array([tk], dtype=np.uint32).view(np.float32)[0]
    nc = int((a >= tau * CAND_MARGIN).sum())
    return nc, regime_of(nc, shape, k), float(tau)


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
class Case(NamedTuple):
    train: List[str]
    test: List[str]
    labels: List[str]
    info: Dict

    @property
    def lines(self):
        return self.train, self.test, self.labels


ANCHOR = "zz_anchor"  # sorts after every s#####: the highest song id


def song(i: int) -> str:
    return f"s{i:05d}"


def _tsv(user: str, name: str) -> str:
    return f"{user}\t{name}\t1"


def _anchored(listeners: Dict[int, int], n_named: int, extra_test: Sequence[str] = ()) -> Tuple[List[str], List[str], List[str]]:
    """Test user X hears the anchor only; train user a<v> hears the anchor and
    every song s with listeners[s] > v (a000 hears every song: the background,
    one anchor listener each). ibm: score ~ C / sqrt(c); ubm: the sum of the
    first C anchor listeners' weights, so it grows with C."""
    n_anchor = max(listeners.values(), default=1)
    train = []
    for v in range(n_anchor):
        train.append(_tsv(f"a{v:03d}", ANCHOR))
        ids = range(n_named) if v == 0 else sorted(s for s, c in listeners.items() if c > v)
        train += [_tsv(f"a{v:03d}", song(s)) for s in ids]
    return train, [_tsv("X", ANCHOR)] + list(extra_test), [_tsv("X", song(0))]


def packed_rows(nt: int, ng: int, tile: int, k: int, m: int, *, block: int, n_tiles: int, tied: bool = False,
                spice: int = 3, seed: int = 0) -> Case:
    """The best m songs of tile `tile` sit on tile-local indices owned by k - 1
    threshold rows (rows 1 .. k-1), shuffled over them; one pivot song in row k
    beats the background, so tau is the pivot and nc = m + 1. tied=False: the
    m songs have distinct scores (song of rank j has A - j anchor listeners);
    tied=True: one score. A few songs of the same ladder (`spice` per other
    tile, the odd ranks) live in the other tiles so that the merged list draws
    from every tile. The last tile is partial and odd-sized."""
    assert 2 <= k <= ng and 0 <= tile < n_tiles
    gs = nt // ng
    n_named = (n_tiles - 1) * block + block // 2 + 2  # + the anchor: the last id
    blo = tile * block
    bw = min(block, n_named - blo)
    idx = np.arange(bw)
    thread = idx % nt
    row = thread // gs
    slots = [int(i) for i in idx if 1 <= row[i] <= k - 1]
    slots.sort(key=lambda i: (i // nt, int(thread[i]) % gs, int(row[i])))  # every row gets a song first
    assert k - 1 <= m <= len(slots), (m, len(slots))
    pivot = blo + (k % ng) * gs
    assert pivot < blo + bw
    spice_ids = []
    for t in range(n_tiles):
        if t != tile:
            spice_ids += [s for s in (t * block + 5 + 41 * i for i in range(spice)) if s < min((t + 1) * block, n_named)]
    spice_ids = spice_ids[:m]
    total = m + len(spice_ids)
    ranks = list(range(total))
    spice_ranks = ranks[1::2][:len(spice_ids)]
    packed_ranks = [r for r in ranks if r not in set(spice_ranks)]
    rng = np.random.default_rng(seed)
    rng.shuffle(packed_ranks)
    n_anchor = 5 if tied else total + 2
    rank_of = {blo + slots[i]: r for i, r in enumerate(packed_ranks)}
    rank_of.update(dict(zip(spice_ids, spice_ranks)))
    listeners = {s: (n_anchor if tied else n_anchor - r) for s, r in rank_of.items()}
    listeners[pivot] = 2
    train, test, labels = _anchored(listeners, n_named)
    return Case(train, test, labels, dict(tile=tile, blo=blo, bhi=blo + bw, pivot=pivot, nc=m + 1, block=block,
                                          n_tiles=n_tiles, n_songs=n_named + 1, user=0,
                                          packed=sorted(blo + s for s in slots[:m])))


def tie_flood(m: int, *, stride: int = 17, level: int = 6) -> Case:
    """m songs (ids 3 + stride * i: spread over the threshold rows) with the
    same listeners, hence an identical (accumulator, c) and one positive score,
    above a lower background (one anchor listener each)."""
    n_named = 3 + m * stride + 40
    flood = [3 + stride * i for i in range(m)]
    train, test, labels = _anchored({s: level for s in flood}, n_named)
    return Case(train, test, labels, dict(flood=flood, n_songs=n_named + 1, user=0))


def boundary_cuts(c_tr: np.ndarray, n_shards: int) -> List[int]:
    """The interior cuts of sharding.song_shards (equal sums of c_tr + 1)."""
    cost = np.cumsum(c_tr.astype(np.int64) + 1)
    total = int(cost[-1])
    n = c_tr.shape[0]
    bounds = [0]
    for g in range(1, n_shards):
        b = int(np.searchsorted(cost, total * g / n_shards, side="left")) + 1
        bounds.append(min(max(b, bounds[-1] + 1), n - (n_shards - g)))
    return bounds[1:]


def boundary_ties(block: int, n_tiles: int, *, group: int = 6, n_shards: int = 3, shard_group: int = 12) -> Case:
    """Equal-score groups of `group` consecutive songs astride every tile
    boundary t * block (5 anchor listeners at odd t, 4 at even t) and groups
    of `shard_group` songs (3 listeners) astride the cuts of
    song_shards(ds, n_shards). The lists are then filled in song-id order
    within a level, across tiles; with group = 6 the k-th place falls inside a
    group for k = 1, 4, 10, 16 (3 tiles) and for 16 / 64 with many tiles."""
    n_named = (n_tiles - 1) * block + block // 2 + 2
    listeners: Dict[int, int] = {}
    groups = []
    for t in range(1, n_tiles):
        lo, hi = t * block - group // 2, t * block + group // 2
        lvl = 5 if t % 2 else 4
        groups.append((lo, hi, lvl))
        listeners.update({s: lvl for s in range(lo, hi)})

    def c_train():
        c = np.ones(n_named + 1, dtype=np.int64)
        for s, lv in listeners.items():
            c[s] = lv
        c[n_named] = 5  # the anchor
        return c

    for cut in boundary_cuts(c_train(), n_shards):
        lo, hi = cut - shard_group // 2, cut + shard_group // 2
        if any(s in listeners for s in range(lo - 1, hi + 1)) or lo < 1 or hi >= n_named:
            continue  # the cut already sits at a tile-boundary group
        groups.append((lo, hi, 3))
        listeners.update({s: 3 for s in range(lo, hi)})
    assert n_tiles >= 2  # the group at the first boundary has the 5 anchor listeners c_train() assumes
    train, test, labels = _anchored(listeners, n_named)
    return Case(train, test, labels, dict(groups=sorted(groups), block=block, n_tiles=n_tiles, n_songs=n_named + 1,
                                          n_shards=n_shards, user=0))


# ---- near ties of the ItemBasedModel ---------------------------------------
NEAR_A = 40          # anchor listeners per family; a family's anchor has c = NEAR_A + 1
NEAR_CMAX = 400      # c(s) of a pair member at most
FAMILIES = ("invert", "equal_approx", "equal_key", "int_near", "control")


def near_tie_pairs(frac_bits: int = 32, per_family: int = 2) -> Dict[str, List[Tuple[Tuple[int, int], Tuple[int, int]]]]:
    """Pairs ((C1, c1), (C2, c2)) of (co-listeners, song count) for one test
    song with c = NEAR_A + 1, searched with the approximation model; the first
    member is the better one (higher fp64 key; for equal keys, the one whose
    approximation is lower, which the generator gives the lower song id).
      invert        key1 > key2, approximation a1 < a2
      equal_approx  key1 > key2, a1 == a2
      equal_key     key1 == key2 from different (C, c): rational ties
                    (C j) / sqrt(c j^2) whose fp64 quotients coincide
      int_near      C1^2 c2 - C2^2 c1 = +-1 with a relative gap below 2^-17
      control       adjacent scores with a relative gap in (2^-17, 2^-15)
    Cheapest pairs (smallest c1 + c2) first."""
    q = int(np.rint(2.0 ** frac_bits / np.sqrt(float(NEAR_A + 1))))
    C, c = np.meshgrid(np.arange(1, NEAR_A), np.arange(1, NEAR_CMAX + 1), indexing="ij")
    ok = c >= C
    C, c = C[ok], c[ok]
    acc = C.astype(np.int64) * q
    score = exact_scores(acc, c, True, frac_bits)
    key = score.view(np.int64)
    a = approx_f32(acc, c, True)
    order = np.lexsort((c, -key))
    C, c, key, a, score = C[order], c[order], key[order], a[order], score[order]
    out: Dict[str, list] = {f: [] for f in FAMILIES}
    i, j = np.arange(key.shape[0] - 1), np.arange(1, key.shape[0])
    rel = (score[i] - score[j]) / score[j]
    det = C[i].astype(np.int64) ** 2 * c[j] - C[j].astype(np.int64) ** 2 * c[i]

    def take(name, mask, flip=None):
        idx = np.flatnonzero(mask)
        idx = idx[np.argsort((c[idx] + c[idx + 1]), kind="stable")]
        for t in idx[:per_family]:
            p, r = ((int(C[t]), int(c[t])), (int(C[t + 1]), int(c[t + 1])))
            out[name].append((r, p) if flip is not None and flip[t] else (p, r))

    take("invert", (key[i] > key[j]) & (a[i] < a[j]))
    take("equal_approx", (key[i] > key[j]) & (a[i] == a[j]))
    take("equal_key", (key[i] == key[j]) & (a[i] != a[j]), flip=a[i] > a[j])
    if not out["equal_key"]:
        take("equal_key", key[i] == key[j])
    take("control", (rel > 2.0 ** -17 * 1.05) & (rel < 2.0 ** -15))
    # int_near pairs need not be adjacent: search every (C1, C2, c1)
    near = []
    for c1v in range(2, NEAR_A):
        for c2v in range(1, c1v):
            cc1 = np.arange(c1v, NEAR_CMAX + 1, dtype=np.int64)
            for sgn in (1, -1):
                num = c2v * c2v * cc1 + sgn  # C1^2 c2 = C2^2 c1 + sgn
                hit = (num % (c1v * c1v) == 0)
                for x1, x2 in zip(cc1[hit], num[hit] // (c1v * c1v)):
                    if c2v <= x2 <= NEAR_CMAX:
                        near.append(((c1v, int(x1)), (c2v, int(x2))))
    near.sort(key=lambda pr: pr[0][1] + pr[1][1])
    for p, r in near:
        sp, sr = (float(exact_scores(np.array([x[0] * q]), np.array([x[1]]), True, frac_bits)[0]) for x in (p, r))
        if sp != sr and abs(sp - sr) / min(sp, sr) < 2.0 ** -17:
            out["int_near"].append((p, r) if sp > sr else (r, p))
        if len(out["int_near"]) >= per_family:
            break
    return out


def near_ties(k: int, *, frac_bits: int = 32, stride: int = 17) -> Case:
    """ibm data, one test user per pair of near_tie_pairs(): the user's anchor
    song is heard by its own NEAR_A train users, k - 1 strong songs (all of
    them listen) fill the first k - 1 places, the pair's better member is the
    k-th and the other the (k + 1)-th. Every song of a user sits in its own
    threshold row (ids `stride` apart), so the candidate path's tau is the
    better approximation of the pair. c(s) above C(s) comes from duplicate
    lines of one more test user. Other songs score 0 for the user."""
    pairs = near_tie_pairs(frac_bits)
    fam = [(name, p, r) for name in FAMILIES for p, r in pairs[name]]
    span = (k + 2) * stride
    n_named = len(fam) * span + 7
    train, test, used = [], [], set()
    info = []
    for f, (name, p, r) in enumerate(fam):
        anchor = f"zz_a{f:02d}"
        users = [f"g{f:02d}_{v:02d}" for v in range(NEAR_A)]
        train += [_tsv(u, anchor) for u in users]
        test.append(_tsv(f"x{f:02d}", anchor))
        base = f * span + 3
        strong = [base + stride * j for j in range(k - 1)]
        s1, s2 = base + stride * (k - 1), base + stride * k
        # the better member gets the lower id when the keys tie; otherwise alternate
        first, second = (p, r) if (name == "equal_key" or f % 2 == 0) else (r, p)
        members = [(s, NEAR_A, NEAR_A) for s in strong] + [(s1, *first), (s2, *second)]
        for s, cl, cnt in members:
            used.add(s)
            train += [_tsv(u, song(s)) for u in users[:cl]]
            test += [_tsv("ydup", song(s))] * (cnt - cl)
        better, worse = (s1, s2) if first == p else (s2, s1)
        info.append(dict(family=name, user=f, strong=strong, better=better, worse=worse, pair=(p, r)))
    train += [_tsv("bg", song(s)) for s in range(n_named) if s not in used]
    if not any(ln.startswith("ydup\t") for ln in test):
        test.append(_tsv("ydup", song(0)))
    return Case(train, test, [_tsv("x00", song(0))], dict(families=info, n_songs=n_named + len(fam), k=k,
                                                          frac_bits=frac_bits))


# ---------------------------------------------------------------------------
# the packed_rows cases of tests/test_gpu_topk_adversarial.py; the regime each
# one names is asserted from the oracle's keys (CPU file, and again on the GPU)
# ---------------------------------------------------------------------------
class Packed(NamedTuple):
    name: str
    shape: str      # "fused" (also run as "separate") or "wide"
    k: int
    block: int
    n_tiles: int
    tile: int
    m: int
    tied: bool
    regime: str


PACKED = [
    # fused / separate: NT = 256, 32 rows of 8 threads, cap 256
    Packed("f-k10-nc10", "fused", 10, 768, 3, 1, 9, False, "parallel"),
    Packed("f-k10-nc125", "fused", 10, 768, 3, 1, 124, False, "parallel"),
    Packed("f-k10-nc126", "fused", 10, 768, 3, 1, 125, True, "parallel"),
    Packed("f-k10-nc127", "fused", 10, 768, 3, 1, 126, False, "parallel"),
    Packed("f-k10-nc128", "fused", 10, 768, 3, 1, 127, False, "parallel"),
    Packed("f-k10-nc129", "fused", 10, 768, 3, 1, 128, False, "one_wave"),
    Packed("f-k10-nc217", "fused", 10, 768, 3, 1, 216, False, "one_wave"),  # nine whole rows of 24 songs
    Packed("f-k10-nc217-tied", "fused", 10, 768, 3, 1, 216, True, "one_wave"),
    Packed("f-k16-nc256", "fused", 16, 1024, 3, 1, 255, False, "one_wave"),
    Packed("f-k16-nc257", "fused", 16, 1024, 3, 1, 256, False, "overflow"),  # -> block_topk
    Packed("f-k16-nc301-tied", "fused", 16, 1024, 3, 1, 300, True, "overflow"),
    Packed("f-k10-wide-tile", "fused", 10, 8192, 2, 0, 300, False, "overflow"),  # -> block_topk_wide
    Packed("f-k16-wide-tile-tied", "fused", 16, 8192, 2, 0, 300, True, "overflow"),
    # wide: NT = 1024, 64 rows of 16 threads, cap min(256, 16 k)
    Packed("w-k2-nc2", "wide", 2, 4096, 2, 0, 1, False, "parallel"),
    Packed("w-k2-nc32", "wide", 2, 4096, 2, 0, 31, False, "parallel"),
    Packed("w-k2-nc41", "wide", 2, 4096, 2, 0, 40, False, "overflow"),
    Packed("w-k10-nc128", "wide", 10, 2048, 3, 1, 127, False, "parallel"),
    Packed("w-k10-nc129", "wide", 10, 2048, 3, 1, 128, False, "one_wave"),
    Packed("w-k10-nc160-tied", "wide", 10, 2048, 3, 1, 159, True, "one_wave"),
    Packed("w-k10-nc161", "wide", 10, 2048, 3, 1, 160, False, "overflow"),
    Packed("w-k16-nc256", "wide", 16, 2048, 3, 1, 255, False, "one_wave"),
    Packed("w-k16-nc257", "wide", 16, 2048, 3, 1, 256, False, "overflow"),
    Packed("w-k16-nc257-tied", "wide", 16, 2048, 3, 1, 256, True, "overflow"),
]


def packed_case(p: Packed) -> Case:
    s = SHAPES[p.shape]
    return packed_rows(s.nt, s.ng, p.tile, p.k, p.m, block=p.block, n_tiles=p.n_tiles, tied=p.tied)
