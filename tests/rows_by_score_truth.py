"""Host truth for eps_rows_by_score (csrc/rows_by_score.hip), in numpy: the cut and the selection count of a re-scored list -- the
definition of eps_score_hist + eps_score_pick_compact with above = base = bar, restated from csrc/score_buckets.h -- and the rows
of the selection in the declared order (score descending, then (v, u) ascending in the caller's labels)."""
import numpy as np

TS_MB = 8                           # mantissa bits of the bucket minifloat (csrc/score_buckets.h)


def ordered(f) -> int:
    """Order-preserving uint32 of a float32 (-0 as +0)."""
    b = int((np.float32(f) + np.float32(0.0)).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def unordered(o: int) -> np.float32:
    b = (o & 0x7FFFFFFF) if o & 0x80000000 else (~o & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


def bucket(d: int) -> int:
    """Bucket of a distance d >= 0: d itself below 2^MB, else exponent | top MB mantissa bits."""
    if d < 1 << TS_MB:
        return d
    e = d.bit_length() - 1
    return ((e - TS_MB + 1) << TS_MB) | ((d >> (e - TS_MB)) & ((1 << TS_MB) - 1))


def bucket_floor(b: int) -> int:
    """Smallest distance that falls into bucket b."""
    if b < 1 << TS_MB:
        return b
    e1, m = b >> TS_MB, b & ((1 << TS_MB) - 1)
    return ((1 << TS_MB) | m) << (e1 - 1)


def cut_and_count(vals: np.ndarray, bar, k2: int):
    """(cut float32, n_sel, live mask & selected mask) of a list of scores: live = above the bar and above -inf; fewer than k2 live
    entries (or k2 = 0): cut = -inf and every live entry is selected; else the cut is the lower edge of the bucket, of distances to
    the bar, that holds the k2-th best live score, and the live entries at or above it are selected."""
    vals = np.asarray(vals, np.float32)
    bar = np.float32(bar)
    live = (vals > bar) & (vals > -np.inf)
    cut = np.float32(-np.inf)
    if k2 != 0 and int(live.sum()) >= k2:
        x = np.sort(vals[live])[::-1][k2 - 1]
        ob, o = ordered(bar), ordered(x)
        b = bucket(o - ob if o > ob else 0)
        if b != 0:
            cut = unordered(min(ob + bucket_floor(b), 0xFFFFFFFF))
    sel = live & (vals >= cut)
    return cut, int(sel.sum()), sel


def ordered_rows(keys_vu: np.ndarray, vals: np.ndarray, k: int, perm=None):
    """The first min(k, 2 m) directed rows of m unordered pairs (keys v << 32 | u, scores): (pairs int64 [2, take] as (u; v), scores).
    Ids go through ``perm`` first (id i is the caller's perm[i]); both orientations of a pair carry its score."""
    keys_vu = np.asarray(keys_vu, np.int64)
    vals = np.asarray(vals, np.float32)
    a, b = keys_vu & 0xFFFFFFFF, keys_vu >> 32
    if perm is not None:
        a, b = np.asarray(perm, np.int64)[a], np.asarray(perm, np.int64)[b]
    u, v, s = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([vals, vals])
    o = np.lexsort((u, v, -s.astype(np.float64)))             # last key first: score descending, then v, then u
    o = o[:min(int(k), o.size)]
    return np.stack([u[o], v[o]]), s[o]


def rows_by_score(keys_by_u: np.ndarray, vals: np.ndarray, bar, k2: int, k: int, perm=None):
    """What eps_rows_by_score computes from a re-scored list (keys u << 32 | v): (cut, n_sel, pairs, scores, longest run of equal
    scores among the selected pairs)."""
    keys_by_u = np.asarray(keys_by_u, np.int64)
    vals = np.asarray(vals, np.float32)
    cut, n_sel, sel = cut_and_count(vals, bar, k2)
    ku = keys_by_u[sel]
    keys_vu = ((ku & 0xFFFFFFFF) << 32) | (ku >> 32)
    pairs, scores = ordered_rows(keys_vu, vals[sel], k, perm)
    longest = int(np.unique(vals[sel], return_counts=True)[1].max()) if n_sel else 0
    return cut, n_sel, pairs, scores, longest
