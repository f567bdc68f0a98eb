"""Model quality over engine outputs (host side; the scores come from the GPU).

* ``threshold_map`` — the reference's evaluateModel (MusicRecommender.scala
  MR:521-639): global min/max normalisation (MR:524-525), prediction if the
  normalised score is > t for t in 0.0..0.9 (MR:529, MR:590), per new-song
  confusion over the test users (MR:541-553), AP(g) = Σ_{i<8} (R_i−R_{i+1})·P_i
  + R_8·P_8 + 0 (MR:601-609), mAP = Σ AP / |newSongs| (MR:626).
* ``map_at_k`` — the build-defined mAP@k over the engine's top-k lists
  (SURVEY.md §8d): AP@k(u) = Σ_{i<=k} P@i·rel(i) / min(k, |labels(u)|).
* ``rank_lists`` — the numpy restatement of the engine's full ranked lists
  (mr_rank_dense_device): per user the K best valid entries by (value desc,
  song id asc).
* ``song_similarity`` / ``similar_lists`` — the numpy restatement of the
  similar-song query (mr_similar_songs_device): the reference's
  cosineSimilarity (MR:230-239) rows of query songs and their top-K lists.
* ``asym_item_model`` — the numpy restatement of the asymmetric-cosine,
  locality-q item-based model (mr_ibm_asym_device), tables from the library's
  host-only mr_asym_tables.
* ``asym_user_keys`` / ``asym_user_model`` — the numpy restatement of the
  asymmetric-cosine, locality-q user-based model (mr_ubm_asym_device):
  fixed-point neighbour weights from the same tables, int64 sums.
Vectorised over the dense n_test x n_songs score matrix (NaN = no pair).
"""
from __future__ import annotations

import numpy as np

from .dataset import Dataset

THRESHOLDS = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)  # MR:590
# the distributed evaluation's 11 thresholds (distributed.scala:395)
THRESHOLDS_DISTRIBUTED = THRESHOLDS + (1.0,)


def label_matrix(ds: Dataset) -> np.ndarray:
    m = np.zeros((ds.n_test, ds.n_songs), dtype=bool)
    rows = np.repeat(np.arange(ds.n_test), np.diff(ds.lab_off))
    keep = ds.lab_songs < ds.n_songs          # label-only songs are never predicted
    m[rows[keep], ds.lab_songs[keep]] = True
    return m


def label_pos(ds: Dataset) -> np.ndarray:
    """pos[s] = #test users whose labels hold song s (TP + FN of class s), s < n_songs."""
    keep = ds.lab_songs < ds.n_songs
    return np.bincount(ds.lab_songs[keep], minlength=ds.n_songs).astype(np.int32)


def threshold_counts(scores: np.ndarray, ds: Dataset, mn: float, mx: float, thresholds=THRESHOLDS):
    """(pred, tp), each n_songs x len(thresholds): per song and threshold, the test users
    predicted ((x - mn)/(mx - mn) > t, MR:529) and those of them whose labels
    hold the song (MR:541-553). The numpy twin of mr_eval_counts_device."""
    x = np.asarray(scores, dtype=np.float64)
    valid = ~np.isnan(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = (x - mn) / (mx - mn)
    lab = label_matrix(ds)
    pred = np.zeros((x.shape[1], len(thresholds)), dtype=np.int64)
    tp = np.zeros_like(pred)
    for i, t in enumerate(thresholds):
        with np.errstate(invalid="ignore"):
            p = valid & (norm > t)             # NaN > t is False (MR:529)
        pred[:, i] = p.sum(axis=0)
        tp[:, i] = (p & lab).sum(axis=0)
    return pred, tp


def map_from_counts(pred: np.ndarray, tp: np.ndarray, pos: np.ndarray, n_label_songs: int) -> float:
    """AP per class (MR:588-618) and the mean (MR:625-627) from the counts:
    P_i = TP/(TP+FP), R_i = TP/(TP+FN) (MR:563-581), with n = pred.shape[1]
    thresholds AP = Σ_{i<n-2} (R_i−R_{i+1})·P_i + R_{n-2}·P_{n-2} + 0 (left
    fold; n = 10 MR:601-609, n = 11 distributed.scala:405-413), classes summed
    in song-id order."""
    if n_label_songs == 0:
        return float("nan")
    pred = np.asarray(pred, dtype=np.float64)
    tp = np.asarray(tp, dtype=np.float64)
    pos = np.asarray(pos)
    n = pred.shape[1]
    P = [np.where(pred[:, i] > 0, tp[:, i] / np.maximum(pred[:, i], 1), 0.0) for i in range(n)]
    R = [np.where(pos > 0, tp[:, i] / np.maximum(pos, 1), 0.0) for i in range(n)]
    ap = np.zeros(pred.shape[0])
    for i in range(n):                         # List.sum: left fold in threshold order
        if i == n - 1:
            term = 0.0
        elif i == n - 2:
            term = (R[i] - 0.0) * P[i]
        else:
            term = (R[i] - R[i + 1]) * P[i]
        ap = ap + term
    total = 0.0
    for v in ap[pos > 0]:                      # other newSongs have AP = 0
        total += float(v)
    return total / n_label_songs


def threshold_map(scores: np.ndarray, ds: Dataset, thresholds=THRESHOLDS) -> float:
    """Reference threshold mAP of a dense model (MR:636), on the host."""
    x = np.asarray(scores, dtype=np.float64)
    valid = ~np.isnan(x)
    if ds.n_label_songs == 0:
        return float("nan")
    mn = x[valid].min()
    mx = x[valid].max()
    pred, tp = threshold_counts(x, ds, mn, mx, thresholds)
    return map_from_counts(pred, tp, label_pos(ds), ds.n_label_songs)


def map_at_k(top_songs: np.ndarray, ds: Dataset, k: int = 10) -> float:
    """Build-defined mAP@k of per-user top-k lists (song -1 = empty slot):
    per test user, Σ_i hit_i · (hits up to i) / i over the first k slots,
    divided by min(k, |distinct labels|); users without labels count 0.
    Vectorised: membership of every (user, song) slot in the user's label set
    by one binary search over the sorted (user, song) label keys."""
    n_te = ds.n_test
    if n_te == 0:
        return 0.0
    top = np.asarray(top_songs)[:, :k].astype(np.int64)
    lab_off = np.asarray(ds.lab_off, dtype=np.int64)
    lab = np.asarray(ds.lab_songs, dtype=np.int64)
    m = int(max(int(lab.max()) if lab.size else 0, int(top.max()) if top.size else 0)) + 1
    lab_user = np.repeat(np.arange(n_te, dtype=np.int64), np.diff(lab_off))
    keys = np.unique(lab_user * m + lab)  # distinct labels per user (set semantics)
    n_lab = np.bincount(keys // m, minlength=n_te)
    q = np.arange(n_te, dtype=np.int64)[:, None] * m + np.maximum(top, 0)
    pos = np.minimum(np.searchsorted(keys, q), max(keys.size - 1, 0))
    hit = (top >= 0) & (keys.size > 0) & (keys[pos] == q) if keys.size else np.zeros_like(top, dtype=bool)
    ranks = np.arange(1, top.shape[1] + 1, dtype=np.float64)
    ap = (hit * (np.cumsum(hit, axis=1) / ranks)).sum(axis=1)
    denom = np.minimum(k, n_lab)
    return float(np.where(denom > 0, ap / np.maximum(denom, 1), 0.0).sum() / n_te)


def rank_lists(dense: np.ndarray, K: int, song_lo: int = 0):
    """(songs int32, scores float64), each n_users x K: per row of a dense model
    (NaN = no pair) the K valid entries with the highest stored value, ordered
    by (value desc, song id = song_lo + column asc); -0.0 ranks and is returned
    as +0.0; missing slots hold -1 / NaN. The numpy twin of
    mr_rank_dense_device (f32 values widen to float64 exactly)."""
    d = np.asarray(dense)
    if d.ndim != 2 or K < 1:
        raise ValueError("rank_lists: a 2-d model and K >= 1")
    songs = np.full((d.shape[0], K), -1, dtype=np.int32)
    scores = np.full((d.shape[0], K), np.nan, dtype=np.float64)
    for u in range(d.shape[0]):
        cols = np.nonzero(~np.isnan(d[u]))[0]
        vals = d[u, cols].astype(np.float64) + 0.0  # -0.0 + 0.0 = +0.0
        order = np.lexsort((cols, -vals))[:K]       # value desc, then column asc
        songs[u, :order.size] = cols[order] + song_lo
        scores[u, :order.size] = vals[order]
    return songs, scores


def song_similarity(ds: Dataset, queries, song_lo: int = 0, song_hi=None) -> np.ndarray:
    """cosineSimilarity(q, s) (MR:230-239) of every query song (global ids,
    repeats allowed) against the songs [song_lo, song_hi): float64 rows
    len(queries) x (song_hi - song_lo). The numerator is the number of distinct
    train users who heard both (from the train CSR: test users never count,
    repeated lines count once); the value is num / (sqrt(c(q)) * sqrt(c(s)))
    with c = song_count (train and test lines, duplicates counted), 0.0 for a
    zero denominator; the entry s == q is NaN (the reference skips s2 == song).
    The numpy twin of mr_similar_songs_device's dense rows, the CPU definition
    the device is compared against bit for bit."""
    song_hi = ds.n_songs if song_hi is None else int(song_hi)
    song_lo = int(song_lo)
    q = np.asarray(queries, dtype=np.int64).reshape(-1)
    if q.size and (q.min() < 0 or q.max() >= ds.n_songs):
        raise ValueError("song_similarity: query ids must be in [0, n_songs)")
    if not 0 <= song_lo <= song_hi <= ds.n_songs:
        raise ValueError("song_similarity: bad song range")
    tr_off = np.asarray(ds.tr_off, dtype=np.int64)
    tr_songs = np.asarray(ds.tr_songs, dtype=np.int64)
    users = np.repeat(np.arange(ds.n_train, dtype=np.int64), np.diff(tr_off))
    sq = np.sqrt(np.asarray(ds.song_count, dtype=np.float64))
    out = np.empty((q.size, song_hi - song_lo), dtype=np.float64)
    rows = {}
    for i, qs in enumerate(q.tolist()):
        if qs not in rows:
            heard = np.zeros(ds.n_train, dtype=bool)
            heard[users[tr_songs == qs]] = True             # L_tr(q)
            num = np.bincount(tr_songs[heard[users]], minlength=ds.n_songs)[song_lo:song_hi].astype(np.float64)
            den = np.sqrt(np.float64(ds.song_count[qs])) * sq[song_lo:song_hi]
            with np.errstate(invalid="ignore", divide="ignore"):
                row = np.where(den != 0, num / den, 0.0)
            if song_lo <= qs < song_hi:
                row[qs - song_lo] = np.nan
            rows[qs] = row
        out[i] = rows[qs]
    return out


def asym_tables(alpha: float, counts) -> tuple:
    """(pow_a, pow_b) = (c^alpha, c^(1-alpha)) as float64 arrays from the
    engine library's host-only mr_asym_tables (it loads without a GPU): the
    very values the device reads, so the twin below does not depend on the libm
    numpy links against."""
    import ctypes

    from . import _lib

    c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    pa = np.empty(c.shape[0], dtype=np.float64)
    pb = np.empty(c.shape[0], dtype=np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(_lib.lib().mr_asym_tables(float(alpha), int(c.shape[0]), p(c), p(pa), p(pb)), "mr_asym_tables")
    return pa, pb


def asym_item_model(ds: Dataset, alpha: float, q: int, song_lo: int = 0, song_hi=None, users=None) -> np.ndarray:
    """The asymmetric-cosine, locality-q item-based model as float64 rows
    n_test x (song_hi - song_lo) (`users`: only those test users' rows, in the
    given order): score(u, s) = the left fold from +0.0, over s2 in T(u) in
    ascending song id, of t = w^q (q - 1 multiplications), w = C(s, s2) /
    (pow_a[s] * pow_b[s2]) with C the distinct train users who heard both
    (from the train CSR), the tables those of mr_asym_tables over song_count,
    0.0 for a zero denominator; NaN for s in T(u). A Python loop over T(u) with
    vector operations over s: the IEEE operation sequence of
    mr_ibm_asym_device, which it is compared against bit for bit. At alpha =
    0.5, q = 1 this is the reference's ItemBasedModel summed literally."""
    song_hi = ds.n_songs if song_hi is None else int(song_hi)
    song_lo, q = int(song_lo), int(q)
    if not 0 <= song_lo <= song_hi <= ds.n_songs:
        raise ValueError("asym_item_model: bad song range")
    if not 1 <= q <= 8:
        raise ValueError("asym_item_model: q must be in [1, 8]")
    pow_a, pow_b = asym_tables(alpha, ds.song_count)
    pa = pow_a[song_lo:song_hi]
    tr_off = np.asarray(ds.tr_off, dtype=np.int64)
    tr_songs = np.asarray(ds.tr_songs, dtype=np.int64)
    deg = np.diff(tr_off)
    order = np.argsort(tr_songs, kind="stable")                      # song -> train listeners
    listeners = np.repeat(np.arange(ds.n_train, dtype=np.int64), deg)[order]
    l_off = np.concatenate([[0], np.cumsum(np.bincount(tr_songs, minlength=ds.n_songs))])
    width = song_hi - song_lo
    terms = {}

    def term(s2: int) -> np.ndarray:
        if s2 not in terms:
            L = listeners[l_off[s2]:l_off[s2 + 1]]                   # L_tr(s2)
            n = deg[L]
            idx = np.repeat(tr_off[L] - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))
            heard = tr_songs[idx]                                     # every listener's distinct songs
            heard = heard[(heard >= song_lo) & (heard < song_hi)] - song_lo
            num = np.bincount(heard, minlength=width).astype(np.float64)   # C(s, s2)
            den = pa * pow_b[s2]
            with np.errstate(invalid="ignore", divide="ignore"):
                w = np.where(den != 0, num / den, 0.0)
            t = w
            for _ in range(q - 1):
                t = t * w
            terms[s2] = t
        return terms[s2]

    rows = range(ds.n_test) if users is None else [int(u) for u in users]
    out = np.empty((len(rows), width), dtype=np.float64)
    for r, u in enumerate(rows):
        mine = np.asarray(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]], dtype=np.int64)
        acc = np.zeros(width, dtype=np.float64)
        for s2 in np.sort(mine).tolist():                            # the fold order
            acc = acc + term(s2)
        acc[mine[(mine >= song_lo) & (mine < song_hi)] - song_lo] = np.nan
        out[r] = acc
    return out


def _asym_user_check(q: int, frac_bits: int) -> None:
    if not 1 <= q <= 8:
        raise ValueError("asym_user_model: q must be in [1, 8]")
    if not 8 <= frac_bits <= 52:
        raise ValueError("asym_user_model: frac_bits must be in [8, 52]")


def _train_listeners(ds: Dataset):
    """(listeners, l_off): the song -> train users CSR of the train CSR."""
    tr_songs = np.asarray(ds.tr_songs, dtype=np.int64)
    deg = np.diff(np.asarray(ds.tr_off, dtype=np.int64))
    order = np.argsort(tr_songs, kind="stable")
    listeners = np.repeat(np.arange(ds.n_train, dtype=np.int64), deg)[order]
    l_off = np.concatenate([[0], np.cumsum(np.bincount(tr_songs, minlength=ds.n_songs))]).astype(np.int64)
    return listeners, l_off


def asym_user_keys(ds: Dataset, alpha: float, q: int, frac_bits: int = 32, users=None) -> list:
    """Per test user (`users`: only those, in the given order) the pair
    (neighbours, keys): the train users v with y = |T(u) ∩ S(v)| >= 1,
    ascending, and their fixed-point weights key = rint(t * 2^frac_bits) as
    int64, t = w^q by q - 1 multiplications, w = y / (pa[u] * pb[v]) (0.0 for a
    zero denominator), pa = te_len^alpha and pb = tr_len^(1-alpha) from
    mr_asym_tables. A key of 0 is a neighbour whose weight is below
    2^-(frac_bits+1): it adds nothing to any score."""
    q, frac_bits = int(q), int(frac_bits)
    _asym_user_check(q, frac_bits)
    pa = asym_tables(alpha, ds.te_len)[0]
    pb = asym_tables(alpha, ds.tr_len)[1]
    listeners, l_off = _train_listeners(ds)
    two_f = np.float64(2.0) ** frac_bits
    out = []
    for u in (range(ds.n_test) if users is None else [int(x) for x in users]):
        mine = np.asarray(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]], dtype=np.int64)
        parts = [listeners[l_off[s2]:l_off[s2 + 1]] for s2 in mine.tolist()]
        heard_by = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        y = np.bincount(heard_by, minlength=ds.n_train)               # distinct songs: both sides are sets
        nb = np.flatnonzero(y)
        den = pa[u] * pb[nb]
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(den != 0, y[nb].astype(np.float64) / den, 0.0)
        t = w
        for _ in range(q - 1):
            t = t * w
        out.append((nb, np.rint(t * two_f).astype(np.int64)))
    return out


def asym_user_model(ds: Dataset, alpha: float, q: int, frac_bits: int = 32, song_lo: int = 0, song_hi=None,
                    users=None) -> np.ndarray:
    """The asymmetric-cosine, locality-q user-based model as float64 rows
    n_test x (song_hi - song_lo) (`users`: only those test users' rows, in the
    given order): score(u, s) = (the int64 sum over the train listeners v of s
    of key(u, v)) * 2^-frac_bits with asym_user_keys' keys; NaN for s in T(u).
    Integer sums over the train CSR rows of u's neighbours (no dense train x
    song matrix), so there is no summation order: the definition
    mr_ubm_asym_device is compared against bit for bit. At alpha = 0.5, q = 1
    this is the engine's fixed-point UserBasedModel (oracle.native.fp_model's
    "ubm") bit for bit."""
    song_hi = ds.n_songs if song_hi is None else int(song_hi)
    song_lo = int(song_lo)
    if not 0 <= song_lo <= song_hi <= ds.n_songs:
        raise ValueError("asym_user_model: bad song range")
    rows = list(range(ds.n_test)) if users is None else [int(u) for u in users]
    keys = asym_user_keys(ds, alpha, q, frac_bits, users=rows)
    tr_off = np.asarray(ds.tr_off, dtype=np.int64)
    tr_songs = np.asarray(ds.tr_songs, dtype=np.int64)
    deg = np.diff(tr_off)
    width = song_hi - song_lo
    inv_f = np.float64(2.0) ** -int(frac_bits)
    out = np.empty((len(rows), width), dtype=np.float64)
    for r, (u, (nb, key)) in enumerate(zip(rows, keys)):
        n = deg[nb]
        idx = np.repeat(tr_off[nb] - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))
        songs = tr_songs[idx]                                         # every neighbour's distinct songs
        add = np.repeat(key, n)
        keep = (songs >= song_lo) & (songs < song_hi)
        acc = np.zeros(width, dtype=np.int64)
        np.add.at(acc, songs[keep] - song_lo, add[keep])
        row = acc.astype(np.float64) * inv_f
        mine = np.asarray(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]], dtype=np.int64)
        row[mine[(mine >= song_lo) & (mine < song_hi)] - song_lo] = np.nan
        out[r] = row
    return out


def similar_lists(dense_rows: np.ndarray, K: int, song_lo: int = 0):
    """(songs int32, scores float64), each n_queries x K, from song_similarity
    rows: the songs with a non-zero cosine (a common train listener) in
    rank_lists' order (cosine desc, song id asc); -1 / NaN padding. The numpy
    twin of mr_similar_songs_device's lists."""
    d = np.array(dense_rows, dtype=np.float64, copy=True)
    d[d == 0] = np.nan  # no common listener: never listed
    return rank_lists(d, K, song_lo)
