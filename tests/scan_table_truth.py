"""The truth the one-pass scan's per-graph tables and plan records are held to (csrc/scan_tables.hip, sp_plan_kernel in
csrc/scan_pieces.hip; the definitions are those of include/eps_abi.h): plain numpy, int64 arithmetic throughout, unsigned
values returned in int64.  A plain helper module (no fixtures, no GPU, no import of the package);
tests/test_scan_tables_host.py validates it on the CPU against brute-force loops, tests/test_gpu_scan_tables.py compares the
HIP kernels with it.

Inputs are ``rowptr`` / ``col`` of a symmetric graph with sorted rows and the other tables as numpy arrays."""
import numpy as np

M = 32
U32 = 0xFFFFFFFF
THREADS_OF = {0: 512, 1: 1024, 2: 256}
BITS_OF = {0: 13, 1: 14, 2: 12}
WIDE = 1 << 24
UBITS = 8192
KIND_HASH, KIND_PACKED, KIND_DIRECT, KIND_DIRECT16 = 0, 1, 2, 3


def _i64(x):
    return np.ascontiguousarray(np.asarray(x)).astype(np.int64)


def unsigned(x):
    """int32 / int16 bits (numpy array) read as unsigned, in int64."""
    x = np.asarray(x)
    mask = {1: 0xFF, 2: 0xFFFF, 4: U32}.get(x.dtype.itemsize)
    return x.astype(np.int64) & mask if mask is not None and x.dtype.kind == "i" else x.astype(np.int64)


def bit_length(x):
    """Bit length of non-negative integers below 2^53 (exact: the exponent of the float64)."""
    return np.frexp(_i64(x).astype(np.float64))[1].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ graphs
def csr_from_edges(n, r, c, keep_loops=False):
    """(rowptr, col) of the symmetric, deduplicated graph with these edges; rows sorted.  Loop-free unless ``keep_loops``: an
    edge (v, v) then stays, as ONE diagonal entry -- an entry like any other, and its own mirror."""
    r, c = _i64(r), _i64(c)
    if not keep_loops:
        keep = r != c
        r, c = r[keep], c[keep]
    key = np.unique(np.concatenate([r * n + c, c * n + r]))
    rows, col = key // n, key % n
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, col.astype(np.int64)


def row_of(rowptr):
    rowptr = _i64(rowptr)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def revpos(rowptr, col):
    """revpos[e] for e = (v, j), w = col[e]: the position of v in row w (the graph is symmetric, rows are sorted).  A diagonal entry
    (v, v) is its own mirror: its revpos is its position in row v, the number of entries of that row below v."""
    rowptr, col = _i64(rowptr), _i64(col)
    n = len(rowptr) - 1
    row = row_of(rowptr)
    # entry keys row * n + col are strictly increasing in CSR order: the mirror (w, v) is found by one search
    mirror = np.searchsorted(row * n + col, col * n + row)
    assert np.array_equal(col[mirror], row) and np.array_equal(row[mirror], col), "the pattern is not symmetric"
    return mirror - rowptr[col]


def half_paths(rowptr, col):
    """Two-hop paths v - w - u with u < v, per column v (a diagonal entry gives the paths v - v - u: they end on known edges)."""
    rowptr, col = _i64(rowptr), _i64(col)
    out = np.zeros(len(rowptr) - 1, np.int64)
    np.add.at(out, row_of(rowptr), revpos(rowptr, col))
    return out


def demo_weights(rowptr):
    """An integer weight table in the 2^-40 fixed point of the exact scores that needs no floating point to state
    (Adamic-Adar-like: 2^40 / (1 + bit length of the degree)); what the plan tests size their sum bounds with."""
    return (1 << 40) // (1 + bit_length(np.diff(_i64(rowptr))))


# ------------------------------------------------------------------------------------------------------------ tables
def bounds(rowptr):
    rowptr = _i64(rowptr)
    n = len(rowptr) - 1
    nnz = int(rowptr[n])
    b = np.zeros(M + 1, np.int64)
    b[M] = n
    ends = rowptr[1:].astype(np.float64)
    for k in range(1, M):
        target = float(k) * (float(nnz) / float(M))
        i = int(np.searchsorted(ends, target, side="left"))          # smallest i with rowptr[i + 1] >= target (n: none)
        b[k] = min(n, i + 1)
    return np.maximum.accumulate(b)


def cuts(rowptr, col, bounds):
    rowptr, col, bounds = _i64(rowptr), _i64(col), _i64(bounds)
    n = len(rowptr) - 1
    # (entry keys row * (n + 1) + id are increasing in CSR order: one search per (row, boundary) counts the ids below it)
    keys = row_of(rowptr) * (n + 1) + col
    below = np.searchsorted(keys, np.arange(n)[:, None] * (n + 1) + bounds[None, 1:], side="left")
    return below - rowptr[:-1, None]


def heads(rowptr, col, fx32, n_hub, budget):
    """[N, 2] (x_v, T_v): the longest prefix of row v with ids < n_hub whose screening weights sum to T_v <= budget."""
    rowptr, col, fx = _i64(rowptr), _i64(col), unsigned(fx32)
    n = len(rowptr) - 1
    out = np.zeros((n, 2), np.int64)
    if not len(col):
        return out
    w = fx[col]
    cs = np.cumsum(w)
    row = row_of(rowptr)
    before = np.concatenate([[0], cs])[rowptr[:-1]]
    t = cs - before[row]                                              # weight of the row's prefix up to and including e
    ok = (col < n_hub) & (t <= budget)
    j = np.arange(len(col)) - rowptr[row]
    deg = np.diff(rowptr)
    stop = np.where(ok, deg[row], j)                                  # position of a failing entry
    x = deg.copy()
    np.minimum.at(x, row, stop)
    out[:, 0] = x
    last = rowptr[:-1] + x - 1
    out[:, 1] = np.where(x > 0, t[np.clip(last, 0, len(col) - 1)], 0)
    return out


def window_paths(rowptr, col, bounds, heads=None, _cuts=None, _revpos=None):
    """(``_cuts`` / ``_revpos``: this module's own tables of the same graph, when the caller has them already.)"""
    rowptr, col, bounds = _i64(rowptr), _i64(col), _i64(bounds)
    n = len(rowptr) - 1
    out = np.zeros((n, M), np.int64)
    if not len(col):
        return out
    ct = cuts(rowptr, col, bounds) if _cuts is None else _cuts
    rev = revpos(rowptr, col) if _revpos is None else _revpos
    row = row_of(rowptr)
    walked = np.ones(len(col), bool)
    if heads is not None:
        walked = np.arange(len(col)) - rowptr[row] >= unsigned(heads)[:, 0][row]
    for lo in range(0, len(col), 1 << 18):
        sl = slice(lo, lo + (1 << 18))
        capped = np.minimum(ct[col[sl]], rev[sl, None])               # entries of row w below bounds[k + 1] AND below v
        per = np.diff(capped, axis=1, prepend=0) * walked[sl, None]
        np.add.at(out, row[sl], per)
    return out


def screen_weights(fixw, shift):
    fixw = _i64(fixw)
    down = 40 - int(shift)
    neg = fixw < 0
    q = (np.where(neg, 0, fixw) + ((1 << down) - 1)) >> down          # (fixw < 2^62: no overflow)
    bad = (1 if neg.any() else 0) | (2 if (q[~neg] > U32).any() else 0)
    fx = np.maximum(1, q & U32)
    fx[neg] = 1
    return fx, bad


def weight_edge_cases(shift):
    """Weights at the rounding edges of a shift: 0, 1, one screening unit and its neighbours and -- where int64 holds them
    (shift >= 10) -- the largest quotient 2^32 - 1, reached exactly and from one below the unit.  -> (fixw, a weight beyond)."""
    one = 1 << (40 - shift)
    w = [0, 1, one - 1, one, one + 1, 3 * one - 1, 3 * one + 1]
    if shift >= 10:
        w += [one * U32, one * U32 - one + 1]
    return np.array(w, np.int64), (one * U32 + 1 if shift >= 10 else None)


def row_sums(rowptr, col, fx32, bounds):
    rowptr, col, fx, bounds = _i64(rowptr), _i64(col), unsigned(fx32), _i64(bounds)
    n = len(rowptr) - 1
    ssum = np.zeros(n, np.int64)
    np.add.at(ssum, row_of(rowptr), fx[col])
    ssum = np.minimum(ssum, (1 << 31) - 1)
    smax = np.zeros(M + 1, np.int64)
    for k in range(M):
        smax[k] = ssum[bounds[k]:].max() if bounds[k] < n else 0
    two = np.diff(rowptr) >= 2
    return ssum, smax, int(fx[two].min()) if two.any() else U32


def row_records(cuts, rowptr, fx32):
    cuts, rowptr, fx = unsigned(cuts), _i64(rowptr), unsigned(fx32)
    n = len(rowptr) - 1
    out = np.zeros((n, 32), np.int64)
    out[:, :16] = cuts[:, 0::2] | (cuts[:, 1::2] << 16)
    out[:, 16] = rowptr[:-1] & U32
    out[:, 17] = fx
    return out


def column_pack(rowptr, col, revpos, rowrec_words, pptr, recs):
    rowptr, col, rev, rr = _i64(rowptr), _i64(col), _i64(revpos), unsigned(rowrec_words)
    pptr, recs = unsigned(pptr), unsigned(recs)
    nnz = len(col)
    out = np.zeros((nnz, 8), np.int64)
    if not nnz:
        return out
    row = row_of(rowptr)
    ct = np.zeros((len(rr), M), np.int64)                             # the cuts, out of the row records' first 16 words
    ct[:, 0::2], ct[:, 1::2] = rr[:, :16] & 0xFFFF, rr[:, :16] >> 16
    npieces = np.diff(pptr)
    c = np.zeros((nnz, 9), np.int64)
    for i in range(9):
        has = np.flatnonzero(npieces[row] > i)                       # entries of columns with a piece i
        k1 = (recs[pptr[row[has]] + i, 1] >> 8) & 0xFF
        c[has, i] = ct[col[has], k1 - 1]
    out[:, 0], out[:, 1], out[:, 2] = col, rr[col, 16], rr[col, 17]
    out[:, 3] = (rev & 0xFFFF) | (c[:, 0] << 16)
    for j in range(4):
        out[:, 4 + j] = c[:, 1 + 2 * j] | (c[:, 2 + 2 * j] << 16)
    return out


# -------------------------------------------------------------------------------------------------------------- plan
def geometry(shift, variant, with_ssum):
    """What the planner reads of the ``variant`` word (geometry in the low byte, (dmax + 1) in byte 1, bit 24 = wide) and the shift."""
    geom, dmax_arg, wide = variant & 0xFF, ((variant >> 8) & 0xFF) - 1, (variant >> 24) & 1
    bits = BITS_OF[geom]
    slots = 1 << bits
    g = dict(variant=geom, bits=bits, slots=slots, direct_ids=2 * slots, piece_paths=slots // 2, packed_paths=slots,
             packed_dmax=min(max(shift - 8, 0), 24), mode_ratio=2270, wide_paths=0, wide_rows=0, pk_on=bool(with_ssum))
    if 0 <= dmax_arg < g["packed_dmax"]:
        g["packed_dmax"] = dmax_arg
    if wide and with_ssum:
        g.update(wide_paths=min(2 << bits, UBITS), wide_rows=THREADS_OF[geom], mode_ratio=8000)
    return g


def plan_column(g, v, dv, bounds, pw, cuts_v, sv=0, smax=None):
    """The pieces of ONE column: sp_plan_column, lane by lane in Python integers.  ``g`` = geometry(...), ``pw`` = wpaths[v],
    ``cuts_v`` = cuts[v], ``sv`` = the column's sum bound without its skipped head.  -> list of (x, y, z, w)."""
    B = [int(b) for b in bounds]
    ek = [0] * (M + 1)
    for k in range(M):
        ek[k + 1] = ek[k] + int(pw[k])
    nbk = [0] + [int(c) for c in cuts_v]
    kv = sum(1 for lane in range(1, M) if B[lane] <= v - 1)
    hi_k = [min(b, v) for b in B]
    recs, k0 = [], 0
    while k0 <= kv:
        lo, e0, nb0 = B[k0], ek[k0], nbk[k0]
        lanes = range(k0 + 1, kv + 2)
        kd = k0 + sum(1 for l in lanes if hi_k[l] - lo <= g["direct_ids"])
        kh = k0 + sum(1 for l in lanes if (ek[l] - e0) + (nbk[l] - nb0) <= g["piece_paths"])
        kp = kd16 = k0
        ms = 0
        if g["pk_on"]:
            ms = min(sv, int(smax[k0]))
            need_s = (ms >> g["packed_dmax"]) + dv + 2
            if need_s < 0x7FFF:
                kd16 = k0 + sum(1 for l in lanes if hi_k[l] - lo <= 2 * g["direct_ids"])
            for l in lanes:
                kb = (max(hi_k[l] - lo, 2) - 1).bit_length()
                cap = 0 if kb >= 30 else (1 << (31 - kb)) - 1
                if (ek[l] - e0) + (nbk[l] - nb0) <= g["packed_paths"] and need_s < cap:
                    kp += 1
            if g["wide_paths"] and dv <= g["wide_rows"]:
                kp = max(kp, k0 + sum(1 for l in lanes if ek[l] - e0 <= g["wide_paths"]))
        kdd = max(kd16, kd)
        take_direct = kdd >= kh and kdd >= kp and kdd > k0
        if not take_direct and kdd > k0 and kp > kdd and kp >= kh:
            pd, pp = ek[kdd] - e0, ek[kp] - e0
            take_direct = (pp - pd) * g["mode_ratio"] < pd * pp
        flag = pq = 0
        if take_direct and kd16 > kd:
            k1, flag, d = kd16, 3 << 30, 0
            while (ms >> d) + dv + 2 >= 0x7FFF:
                d += 1
            pq = d | (16 << 8)
        elif take_direct:
            k1, flag = kd, 2 << 30
        elif kp >= kh and kp > k0:
            k1, flag = kp, 1 << 30
            kb = (max(hi_k[k1] - lo, 2) - 1).bit_length()
            if g["wide_paths"] and dv <= g["wide_rows"]:
                pq = min(kb, 31) << 8
            else:
                cap, d = (1 << (31 - kb)) - 1, 0
                while (ms >> d) + dv + 2 >= cap:
                    d += 1
                pq = d | (kb << 8)
        elif kh > k0:
            k1 = kh
        else:
            k1 = k0 + 1
        paths = ek[k1] - e0
        if paths:
            recs.append((paths | flag, k0 | (k1 << 8) | (pq << 16), nbk[k0] | (nbk[k1] << 16), lo))
        k0 = k1
    return recs


def _sum_bound(n, ssum, heads):
    if ssum is None:
        return np.zeros(n, np.int64)
    ssum = unsigned(ssum)
    return ssum - (np.minimum(unsigned(heads)[:, 1], ssum) if heads is not None else 0)


def plan(rowptr, bounds, cuts, wpaths, ssum, smax, heads, shift, variant, run_slack=2):
    """eps_scan_plan: every column's pieces -- ``plan_column`` for all columns at once (one numpy step per piece index).
    -> (pptr [N + 1], recs [P, 4], d_used).  ``run_slack``: the 2 of the sum bound that sizes a RUN of windows ("need_s": one
    rounding unit per path and the flag bit's neighbour) -- the tests plan with 1 to show that their graphs sit on that edge."""
    rowptr, B, ct, wp = _i64(rowptr), _i64(bounds), unsigned(cuts), unsigned(wpaths)
    n = len(rowptr) - 1
    g = geometry(shift, variant, ssum is not None)
    deg = np.diff(rowptr)
    v = np.flatnonzero((deg > 0) & (np.arange(n) > 0))
    dv = deg[v]
    ek = np.concatenate([np.zeros((len(v), 1), np.int64), np.cumsum(wp[v], axis=1)], axis=1)
    assert not len(v) or ek[:, M].max() < 1 << 31
    nbk = np.concatenate([np.zeros((len(v), 1), np.int64), ct[v]], axis=1)
    hi_k = np.minimum(B[None, :], v[:, None])
    kv = (B[None, 1:M] <= v[:, None] - 1).sum(1)
    sv = _sum_bound(n, ssum, heads)[v]
    smk = unsigned(smax) if smax is not None else np.zeros(M + 1, np.int64)
    L = np.arange(M + 1)[None, :]
    k0 = np.zeros(len(v), np.int64)
    out, seq = [], 0
    while True:
        a = np.flatnonzero(k0 <= kv)
        if not len(a):
            break
        ka, eka, nba, hia, dva = k0[a], ek[a], nbk[a], hi_k[a], dv[a]
        ar = np.arange(len(a))
        lo, e0, nb0 = B[ka], eka[ar, ka], nba[ar, ka]
        inm = (L > ka[:, None]) & (L <= kv[a][:, None] + 1)
        span = np.maximum(hia - lo[:, None], 0)
        paths_to = eka - e0[:, None]
        keys = paths_to + (nba - nb0[:, None])
        kd = ka + (inm & (span <= g["direct_ids"])).sum(1)
        kh = ka + (inm & (keys <= g["piece_paths"])).sum(1)
        kp, kd16, ms = ka.copy(), ka.copy(), np.zeros(len(a), np.int64)
        w_on = np.zeros(len(a), bool)
        if g["pk_on"]:
            ms = np.minimum(sv[a], smk[ka])
            need_s = (ms >> g["packed_dmax"]) + dva + run_slack
            kd16 = np.where(need_s < 0x7FFF, ka + (inm & (span <= 2 * g["direct_ids"])).sum(1), ka)
            kb = bit_length(np.maximum(span, 2) - 1)
            cap = np.where(kb >= 30, 0, (np.int64(1) << np.clip(31 - kb, 0, 31)) - 1)
            kp = ka + (inm & (keys <= g["packed_paths"]) & (need_s[:, None] < cap)).sum(1)
            if g["wide_paths"]:
                w_on = dva <= g["wide_rows"]
                kp = np.where(w_on, np.maximum(kp, ka + (inm & (paths_to <= g["wide_paths"])).sum(1)), kp)
        kdd = np.maximum(kd16, kd)
        take = (kdd >= kh) & (kdd >= kp) & (kdd > ka)
        alt = ~take & (kdd > ka) & (kp > kdd) & (kp >= kh)
        pd, pp = eka[ar, kdd] - e0, eka[ar, kp] - e0
        take |= alt & ((pp - pd) * g["mode_ratio"] < pd * pp)
        c16 = take & (kd16 > kd)
        cd = take & ~c16
        cp = ~take & (kp >= kh) & (kp > ka)
        ch = ~take & ~cp & (kh > ka)
        k1 = np.select([c16, cd, cp, ch], [kd16, kd, kp, kh], ka + 1)
        flag = np.select([c16, cd, cp], [3 << 30, 2 << 30, 1 << 30], 0)
        shifts = np.arange(32)[None, :]
        fits_at = (ms[:, None] >> shifts) + dva[:, None] + 2                  # (minimal d: the count of shifts that do not fit yet)
        d16 = (fits_at >= 0x7FFF).sum(1)
        kb1 = bit_length(np.maximum(hia[ar, k1] - lo, 2) - 1)
        cap1 = (np.int64(1) << np.clip(31 - kb1, 0, 31)) - 1
        dp = (fits_at >= cap1[:, None]).sum(1)
        pq_p = np.where(w_on, np.minimum(kb1, 31) << 8, dp | (kb1 << 8))
        pq = np.select([c16, cp], [d16 | (16 << 8), pq_p], 0)
        paths = eka[ar, k1] - e0
        e = np.flatnonzero(paths > 0)
        rec = np.stack([paths | flag, ka | (k1 << 8) | (pq << 16), nb0 | (nba[ar, k1] << 16), lo], 1)[e]
        out.append((v[a][e], np.full(len(e), seq), rec))
        seq += 1
        k0[a] = k1
    if out:
        vv, ss, recs = (np.concatenate([o[i] for o in out]) for i in range(3))
        order = np.lexsort((ss, vv))
        vv, recs = vv[order], recs[order]
    else:
        vv, recs = np.zeros(0, np.int64), np.zeros((0, 4), np.int64)
    pptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(vv, minlength=n), out=pptr[1:])
    packed = (recs[:, 0] >> 30) & 1 == 1
    d_used = int(((recs[packed, 1] >> 16) & 0xFF).max()) if packed.any() else 0
    return pptr, recs, d_used


def fields(recs):
    r = unsigned(recs).reshape(-1, 4)
    x, y, z, w = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return dict(paths=x & 0x3FFFFFFF, kind=x >> 30, k0=y & 0xFF, k1=(y >> 8) & 0xFF, d=(y >> 16) & 0xFF, kb=(y >> 24) & 0xFF,
                na=z & 0xFFFF, nb=z >> 16, lo=w)


def kind_counts(pptr, recs, rowptr, variant, with_ssum=True):
    """What a plan exercises: pieces per kind, partitioned and wide-packed pieces, columns by their number of pieces."""
    f = fields(recs[:int(unsigned(pptr)[-1])])
    g = geometry(0, variant, with_ssum)
    keys = f["paths"] + f["nb"] - f["na"]
    npieces = np.diff(unsigned(pptr))
    odd = f["kind"] % 2 == 1
    return dict(direct=int((f["kind"] == 2).sum()), direct16=int((f["kind"] == 3).sum()), packed=int((f["kind"] == 1).sum()),
                hash=int(((f["kind"] == 0) & (keys <= g["piece_paths"])).sum()),
                partitioned=int(((f["kind"] == 0) & (keys > g["piece_paths"])).sum()),
                wide_packed=int(((f["kind"] == 1) & (f["paths"] > g["packed_paths"])).sum()) if g["wide_paths"] else 0,
                columns_over_9=int((npieces > 9).sum()), columns_9=int((npieces == 9).sum()),
                columns_1_to_8=int(((npieces >= 1) & (npieces <= 8)).sum()), columns_0=int((npieces == 0).sum()),
                dropped_bits=int(f["d"][odd].max()) if odd.any() else 0)


def check_plan(pptr, recs, d_used, rowptr, bounds, cuts, wpaths, ssum, smax, heads, shift, variant):
    """The invariants of a plan table, asserted from the records alone (this does not run the planner): coverage, fields,
    capacity by kind, d_used.  Raises AssertionError naming the invariant."""
    rowptr, B, ct, wp, pptr = _i64(rowptr), _i64(bounds), unsigned(cuts), unsigned(wpaths), unsigned(pptr)
    n = len(rowptr) - 1
    g = geometry(shift, variant, ssum is not None)
    P = int(pptr[-1])
    f = fields(np.asarray(recs)[:P])
    npieces = np.diff(pptr)
    assert pptr[0] == 0 and (npieces >= 0).all() and len(pptr) == n + 1, "pptr: not a prefix table"
    v = np.repeat(np.arange(n), npieces)
    deg = np.diff(rowptr)
    first = np.ones(P, bool)
    first[1:] = v[1:] != v[:-1]
    k0, k1, paths = f["k0"], f["k1"], f["paths"]
    # 1. coverage
    assert ((k0 < k1) & (k1 <= M)).all(), "coverage: an empty or overlong run"
    assert (first[1:] | (k0[1:] >= k1[:-1])).all(), "coverage: runs overlap or are out of order"
    cw = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(wp, axis=1)], axis=1)
    in_run = cw[v, k1] - cw[v, k0]
    assert (paths > 0).all(), "coverage: a piece without paths"
    assert np.array_equal(paths, in_run), "coverage: a piece's paths are not those of its windows"
    planned = np.zeros(n, np.int64)
    np.add.at(planned, v, paths)
    todo = np.where((deg > 0) & (np.arange(n) > 0), cw[:, M], 0)
    assert np.array_equal(planned, todo), "coverage: paths outside every piece"
    # 2. fields
    assert np.array_equal(f["lo"], B[k0]), "fields: lo"
    assert np.array_equal(f["na"], np.where(k0 > 0, ct[v, np.maximum(k0, 1) - 1], 0)), "fields: na"
    assert np.array_equal(f["nb"], ct[v, k1 - 1]), "fields: nb"
    # 3. capacity by kind
    hi = np.minimum(B[k1], v)
    span = hi - f["lo"]
    keys = paths + f["nb"] - f["na"]
    kind, d, kb = f["kind"], f["d"], f["kb"]
    slots = g["slots"]
    if ssum is None:
        assert np.isin(kind, (0, 2)).all(), "capacity: packed / 16-bit pieces without sum bounds"
        ms = np.zeros(P, np.int64)
    else:
        ms = np.minimum(_sum_bound(n, ssum, heads)[v], unsigned(smax)[k0])
    need = lambda dd: (ms >> np.clip(dd, 0, 62)) + deg[v] + 2
    is_d, is_16, is_p, is_h = kind == 2, kind == 3, kind == 1, kind == 0
    assert (span[is_d] <= 2 * slots).all(), "capacity: a direct piece spans more than 2 x slots ids"
    assert (span[is_16] <= 4 * slots).all() and (kb[is_16] == 16).all(), "capacity: a 16-bit direct piece's span / key bits"
    assert (need(d)[is_16] < 0x7FFF).all(), "capacity: a 16-bit direct piece's sum field overflows"
    assert ((d == 0) | (need(d - 1) >= 0x7FFF))[is_16].all(), "capacity: a 16-bit direct piece drops more bits than it needs"
    want_kb = np.maximum(1, bit_length(np.maximum(span, 1) - 1))
    cap = (np.int64(1) << np.clip(31 - want_kb, 0, 31)) - 1
    sketch = is_p & (deg[v] <= g["wide_rows"]) if g["wide_paths"] else np.zeros(P, bool)
    plain = is_p & ~sketch
    assert (keys[plain] <= slots).all(), "capacity: a packed piece holds more than slots keys"
    assert np.array_equal(kb[plain], want_kb[plain]), "capacity: a packed piece's key bits"
    assert (need(d)[plain] < cap[plain]).all(), "capacity: a packed piece's sum field overflows into its key bits"
    assert ((d == 0) | (need(d - 1) >= cap))[plain].all() and (d[plain] <= g["packed_dmax"]).all(), \
        "capacity: a packed piece drops more bits than it needs or may"
    assert (d[sketch] == 0).all() and np.array_equal(kb[sketch], np.minimum(want_kb, 31)[sketch]), "capacity: a sketch piece's d / key bits"
    assert ((paths <= g["wide_paths"]) | ((keys <= slots) & (need(g["packed_dmax"]) < cap)))[sketch].all(), \
        "capacity: a sketch piece holds more than wide_paths paths"
    assert ((keys <= slots // 2) | (k1 == k0 + 1))[is_h].all(), "capacity: a hash piece over slots / 2 that is no single window"
    # 4. d_used
    odd = (kind & 1) == 1
    assert int(d_used) == (int(d[odd].max()) if odd.any() else 0), "d_used: not the largest d of the packed / 16-bit pieces"


def rewalk(recs, variant):
    """(paths x (parts - 1) over two-word hash pieces beyond a table's capacity, paths of all pieces): eps_scan_plan_rewalk."""
    f = fields(recs)
    cap = (1 << BITS_OF[variant & 0xFF]) // 2
    keys = f["paths"] + f["nb"] - f["na"]
    over = (f["kind"] == 0) & (keys > cap)
    q = (keys + cap - 1) // cap
    parts = np.int64(2) << bit_length(np.maximum(q, 1) - 1)
    return int((f["paths"] * (parts - 1))[over].sum()), int(f["paths"].sum())


# ------------------------------------------------------------------------------------- the graphs the GPU tests use
def relabel(rowptr, col, new_of_old, keep_loops=False):
    """The same graph with node i renamed new_of_old[i] (rows sorted again; diagonal entries are dropped unless ``keep_loops``)."""
    new = _i64(new_of_old)
    return csr_from_edges(len(new), new[row_of(rowptr)], new[_i64(col)], keep_loops)


def hubs_first(rowptr, col, last=False, keep_loops=False):
    """Nodes renamed by falling degree (stable); ``last``: by rising degree, the mirror image.  The degree is the row length: a
    stored diagonal entry counts in it."""
    deg = np.diff(_i64(rowptr))
    order = np.argsort(-deg, kind="stable")
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    return relabel(rowptr, col, len(order) - 1 - inv if last else inv, keep_loops)


def star(leaves, hub_first):
    """A hub with ``leaves`` neighbours of degree one; the hub is id 0 or the last id."""
    hub = 0 if hub_first else leaves
    other = np.arange(1, leaves + 1) if hub_first else np.arange(leaves)
    return csr_from_edges(leaves + 1, np.full(leaves, hub), other)


def lane_stride_graph():
    """133 nodes; the last four have rows of exactly 63, 64, 65 and 129 entries (the first ids are their shared neighbours)."""
    r, c = [], []
    for hub, d in ((129, 63), (130, 64), (131, 65), (132, 129)):
        r += [hub] * d
        c += list(range(d))
    return csr_from_edges(133, r, c)


def small_random(n, m, seed):
    rng = np.random.default_rng(seed)
    return csr_from_edges(n, rng.integers(0, n, m), rng.integers(0, n, m))


PIN_GRAPHS = ("rmat14_hubs_first", "rmat15_hubs_last", "rmat17_as_labelled")
PIN_SHIFT = 18


def pin_graph(synth, name):
    """(rowptr, col) of a graph of the GPU tests, generated on the CPU from ``synth`` (the package's seeded generators; the GPU
    tests upload these arrays, so the host pin of the piece kinds speaks about the very graphs the kernels plan)."""
    scale, factor = {"rmat14_hubs_first": (14, 12), "rmat15_hubs_last": (15, 12), "rmat17_as_labelled": (17, 4)}[name]
    g = synth.rmat_graph(scale, factor, 3, "cpu")
    rp, col = g.rowptr.numpy().astype(np.int64), g.col.numpy().astype(np.int64)
    if name == "rmat14_hubs_first":
        return hubs_first(rp, col)
    if name == "rmat15_hubs_last":
        return hubs_first(rp, col, last=True)
    return rp, col


class Tables:
    """Every table of one graph under demo_weights at PIN_SHIFT, from the truths above."""

    def __init__(self, rowptr, col, shift=PIN_SHIFT, fixw=None):
        self.rowptr, self.col, self.shift = _i64(rowptr), _i64(col), shift
        self.n, self.nnz = len(self.rowptr) - 1, len(self.col)
        self.bounds = bounds(self.rowptr)
        self.cuts = cuts(self.rowptr, self.col, self.bounds)
        self.revpos = revpos(self.rowptr, self.col)
        self.wpaths = window_paths(self.rowptr, self.col, self.bounds, None, self.cuts, self.revpos)
        self.fixw = demo_weights(self.rowptr) if fixw is None else _i64(fixw)
        self.fx32, self.bad = screen_weights(self.fixw, shift)
        self.ssum, self.smax, self.min_fx = row_sums(self.rowptr, self.col, self.fx32, self.bounds)
        self.rowrec = row_records(self.cuts, self.rowptr, self.fx32)
        self._heads = {}

    def head_tables(self, n_hub, budget):
        """(heads, the window paths of the rows still walked) for a head budget; cached."""
        key = (int(n_hub), int(budget))
        if key not in self._heads:
            h = heads(self.rowptr, self.col, self.fx32, n_hub, budget)
            self._heads[key] = (h, window_paths(self.rowptr, self.col, self.bounds, h, self.cuts, self.revpos))
        return self._heads[key]

    def mid_budget(self):
        return 6 * int(self.fx32.max()) if self.n else 0


PLAN_MODES = ("plain", "nosum", "dmax0", "dmax3", "wide", "heads", "heads_wide")


def plan_inputs(t, mode, variant):
    """(wpaths, ssum, smax, heads, variant word) of one way the tests run the planner on the tables ``t``."""
    word = variant | {"dmax0": 1 << 8, "dmax3": 4 << 8, "wide": WIDE, "heads_wide": WIDE}.get(mode, 0)
    wp, hd = t.wpaths, None
    if mode.startswith("heads"):
        hd, wp = t.head_tables(t.n, t.mid_budget())
    ssum, smax = (None, None) if mode == "nosum" else (t.ssum, t.smax)
    return wp, ssum, smax, hd, word
