"""The truth the pair-score kernels (csrc/pair_intersect.hip, csrc/pair_grouped.hip: ops.pair_scores) are held to, and the graphs
and pair lists that put their rows, hit counts and id spaces ON the kernels' switch points.  numpy / scipy only, a plain helper
module (no fixtures); tests/test_pair_score_truth_host.py validates it on the CPU, tests/test_gpu_pair_paths.py compares the HIP
paths with it.  Every builder takes the kernels' limits (ops.pair_scores_limits / pair_scores_grouped_limits) as arguments and
says in a dictionary which case each row or pair was made for.

A graph is a scipy CSR float32 matrix with sorted indices and non-zero stored values; it need not be symmetric."""
import numpy as np
import scipy.sparse as ssp

from cn_list_truth import U, gamma           # noqa: F401  (float32: unit roundoff, gamma_n)

WIDE = np.longdouble
assert np.finfo(WIDE).nmant >= 63, "the truth sums in extended precision"
U64 = 2.0 ** -53
HUB = 40000                                   # the hub every other row meets: far beyond any staging capacity
SPLIT_NUM, SPLIT_DEN = 3, 5                   # the split launch runs when sampled small pairs * 5 > sampled pairs * 3 (eps_abi.h: 60 %)


def gamma64(n):
    """gamma_n of a float64 sum."""
    n = np.asarray(n, np.float64)
    return n * U64 / (1.0 - n * U64)


# ---------------------------------------------------------------------------------------------------------- the truth
def _seg_sum(x, ptr):
    """Sums of the segments x[ptr[i]:ptr[i + 1]] (in the dtype of x), 0 for an empty one."""
    out = np.zeros(len(ptr) - 1, x.dtype)
    full = np.flatnonzero(np.diff(ptr) > 0)
    if len(full):
        out[full] = np.add.reduceat(x, ptr[full])          # (the starts of the non-empty segments ascend strictly and tile x)
    return out


def scores(A, node_w, u, v):
    """-> dict per pair (u[i], v[i]): ``count`` int64 = |N(u) & N(v)| over the stored pattern; ``cn`` float64 = sum of
    A[u,w] A[v,w]; ``ws`` float64 = sum of A[u,w] A[v,w] node_w[w]; ``abs_cn`` / ``abs`` float64 = the sums of the absolute
    terms of cn / ws (the scale of a rounding bound).  Products and sums are formed in extended precision (64-bit mantissa) and
    rounded to float64 ONCE, so ws is within U64 |ws| of the real sum whatever the list length."""
    A = ssp.csr_matrix(A)
    assert A.has_sorted_indices and (A.data != 0).all()
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    P = ssp.csr_matrix((np.ones(A.nnz, np.float64), A.indices, A.indptr), shape=A.shape)
    A64 = A.astype(np.float64)
    Pu, Pv = P[u], P[v]
    X = A64[u].multiply(Pv).tocsr()           # A[u, w] on the common neighbours
    Y = Pu.multiply(A64[v]).tocsr()           # A[v, w] on the common neighbours
    for M in (X, Y):
        M.sort_indices()
    assert np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
    ptr = X.indptr.astype(np.int64)
    t_cn = X.data.astype(WIDE) * Y.data.astype(WIDE)
    t_ws = t_cn * np.asarray(node_w)[X.indices].astype(WIDE)
    f = lambda x: _seg_sum(x, ptr).astype(np.float64)                            # noqa: E731
    return dict(count=np.diff(ptr), cn=f(t_cn), ws=f(t_ws), abs_cn=f(np.abs(t_cn)), abs=f(np.abs(t_ws)))


def frac_bits(x, limit=20):
    """The smallest q with x * 2^q integral everywhere; AssertionError when there is none up to ``limit``."""
    x = np.asarray(x, np.float64)
    for q in range(limit + 1):
        if np.array_equal(np.rint(x * 2.0 ** q), x * 2.0 ** q):
            return q
    raise AssertionError("not dyadic: a stored value or weight is no small multiple of a power of two")


def require_exact(A, node_w, u, v, truth=None):
    """The dyadic family's licence to compare BITS: stored values are multiples of 2^-a, weights of 2^-b, so every term of ws is
    a multiple of 2^-q, q = 2a + b (every term of cn of 2^-2a), and a sum of any subset of the terms in any order stays below
    2^(24 - q) -- then every float32 partial sum is exact whatever the association.  Checked per case (graph, table, list);
    AssertionError when a sum could round.  -> q."""
    a, b = frac_bits(A.data), frac_bits(node_w)
    t = scores(A, node_w, u, v) if truth is None else truth
    q = 2 * a + b
    assert float(np.max(t["abs"], initial=0.0)) < 2.0 ** (24 - q), "a float32 sum of these weighted terms could round"
    assert float(np.max(t["abs_cn"], initial=0.0)) < 2.0 ** (24 - 2 * a), "a float32 sum of these value products could round"
    assert float(np.abs(node_w).max(initial=0.0)) * float(np.abs(A.data).max(initial=0.0)) < 2.0 ** (24 - a - b)
    return q


def dyadic_weights(n, seed=3):
    """k / 32, k in 1 .. 31: 31 distinct values, so a weight gathered from a neighbouring queue slot shows."""
    return (np.random.default_rng(seed).integers(1, 32, n) / 32.0).astype(np.float64)


def real_weights(A, mode, dtype):
    """The AA (1 / log colsum) or RA (1 / colsum) table of A in ``dtype``, inf -> 0 (colsum 0 or 1)."""
    cs = np.asarray(A.astype(np.float64).sum(0)).ravel().astype(dtype)
    with np.errstate(divide="ignore"):
        w = (dtype(1) / np.log(cs)) if mode == "aa" else (dtype(1) / cs)
    w[~np.isfinite(w)] = 0
    return w.astype(dtype)


def unit(A):
    """The same pattern with every stored value 1."""
    return ssp.csr_matrix((np.ones(A.nnz, np.float32), A.indices, A.indptr), shape=A.shape)


def _assemble(n, rows, rng):
    """rows: {id: ids of its entries} -> CSR float32, sorted, values drawn from {0.5, 1, 1.5}."""
    r = np.concatenate([np.full(len(c), i, np.int64) for i, c in rows.items()])
    c = np.concatenate([np.asarray(c, np.int64) for c in rows.values()])
    assert len(c) == 0 or (c.min() >= 0 and c.max() < n)
    flat = np.unique(r * n + c)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(flat // n, minlength=n), out=indptr[1:])
    data = rng.choice(np.array([0.5, 1.0, 1.5], np.float32), len(flat))
    A = ssp.csr_matrix((data, (flat % n).astype(np.int32), indptr), shape=(n, n))
    A.has_sorted_indices = True
    for i, c in rows.items():
        assert indptr[i + 1] - indptr[i] == len(np.unique(c)), i
    return A


# ---------------------------------------------------------------------------------------------------------- generic kernel
def long_lengths(S, C):
    return [1, 2, 3, 4, 5, 63, 64, 65, S - 1, S, S + 1, 256, 257, 512, 513, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 1]


def short_lengths():
    return [0, 1, 15, 16, 17, 63, 64, 65, 129]


def route(du, dv, S, C, R):
    """The way a pair goes through the generic kernel, from its two row lengths: 'empty', 'small' (the sixteen-lane route, where
    the launch is split), 'one' (staged, one pass), 'multi' (staged, several passes), 'inplace'."""
    lo, hi = min(du, dv), max(du, dv)
    if lo == 0:
        return "empty"
    if hi > C and hi >= lo * R:
        return "inplace"
    if hi > C:
        return "multi"
    return "small" if hi <= S else "one"


QUEUE_HITS = ("one", "few", "slice", "open1", "open2")


def queue_hit_counts(Q):
    """Hits of the queue family's pairs: a lone hit, a few, a full 64-entry slice, and two that stay open across one and two
    flushes when they start on a queue of Q - 64."""
    return dict(one=1, few=5, slice=64, open1=3 * 64, open2=Q + 2 * 64)


def generic_graph(S, C, Q, R, seed=11):
    """-> (A, info).  Rows (info['row'][L] = the id of the row with exactly L entries) of every length of long_lengths /
    short_lengths and of (C + 1) // R and (C + 1) // R + 1 -- the two sides of the in-place switch against the row of C + 1 --
    whose first ceil(L / 2) entries are a prefix of one order of the filler ids, so any two of them share entries; a hub; a
    stranger of 64 entries nobody shares.  The row of 513 entries is the LAST row of the matrix and the row of one entry the
    first stored one: the ends of col[] are the end of a staged row.
    info['merge']: a row M of 2C + 1 even ids and shorter rows placed against M[C - 1], the last entry of its first pass.
    info['queue']: a row H and rows T[name] = its first queue_hit_counts()[name] entries, and Z sharing nothing with H."""
    rng = np.random.default_rng(seed)
    lens = sorted(set(long_lengths(S, C)) | set(short_lengths()) | {(C + 1) // R, (C + 1) // R + 1})
    k = len(lens)
    names = ["stranger", "hub", "M", "below", "above", "straddle", "straddle2", "equal", "H", "Z"] + ["T_" + h for h in QUEUE_HITS]
    node = {nm: k + i for i, nm in enumerate(names)}
    f0 = k + len(names)
    m = max(65, (2 * C + 1) // R + 6)                       # a shorter row against M that is staged, not searched in place
    assert route(m, 2 * C + 1, S, C, R) == "multi" and m + 64 < C
    hits = queue_hit_counts(Q)
    h_len = hits["open2"] + 64
    assert S < h_len <= C, "the queue family's long row must be staged in one pass and never take the small route"
    sb, mb = f0, f0 + 64
    hb = mb + 2 * (2 * C + 1)
    pool0 = hb + h_len + 64
    n = pool0 + HUB + 4000
    pool = rng.permutation(np.arange(pool0, n - 1))
    row_of = {L: i for i, L in enumerate(lens)}
    row_of[513] = n - 1                                     # (the id its place in the order would have had keeps an empty row)
    rows = {}

    def shared(L):
        head = (L + 1) // 2
        rest = rng.choice(pool[head:], size=L - head, replace=False) if L > head else np.zeros(0, np.int64)
        return np.concatenate([pool[:head], rest])

    for L in lens:
        rows[row_of[L]] = shared(L)
    rows[node["hub"]] = shared(max(HUB, R * 129 + 1))
    rows[node["stranger"]] = np.arange(sb, sb + 64)
    # the merge family
    M = mb + 2 * np.arange(2 * C + 1)
    last1, last2 = int(M[C - 1]), int(M[2 * C - 1])
    rows[node["M"]] = M
    rows[node["below"]] = mb + np.arange(m)
    rows[node["above"]] = last1 + 1 + np.arange(m)
    rows[node["straddle"]] = np.concatenate([np.arange(last1 - 30, last1), last1 + 1 + np.arange(m - 30)])
    rows[node["straddle2"]] = np.concatenate([np.arange(last1 - 74, last1), last1 + 1 + np.arange(55)])
    rows[node["equal"]] = np.concatenate([np.arange(last1 - 9, last1 + 1), last1 + 1 + np.arange(m), np.arange(last2 - 9, last2 + 1),
                                          [M[2 * C]]])
    # the queue family
    H = hb + np.arange(h_len)
    rows[node["H"]] = H
    rows[node["Z"]] = hb + h_len + np.arange(64)
    for nm, c in hits.items():
        rows[node["T_" + nm]] = H[:c]
    # the filler rows: three random filler entries each (random pairs match now and then, column sums are not all one)
    fill = np.arange(pool0, n - 1)
    extra = rng.integers(pool0, n - 1, (len(fill), 3))
    A = _assemble(n, {**rows, **{int(i): e for i, e in zip(fill, extra)}}, rng)
    deg = np.diff(A.indptr)
    assert all(deg[row_of[L]] == L for L in lens)
    info = dict(n=n, lens=lens, row=row_of, node=node, specials=[row_of[L] for L in lens], m=m, last1=last1, last2=last2,
                first_stored=int(np.flatnonzero(deg)[0]), last_stored=int(np.flatnonzero(deg)[-1]), filler=(pool0, n - 1))
    return A, info


def grid_pairs(info):
    """Every ordered pair of the boundary rows, the hub and the stranger, u == v included -> (u, v) int32."""
    ids = np.array(info["specials"] + [info["node"]["hub"], info["node"]["stranger"]])
    uu, vv = np.meshgrid(ids, ids, indexing="ij")
    return uu.ravel().astype(np.int32), vv.ravel().astype(np.int32)


def merge_pairs(info):
    """The merge family against M, both ways round -> (u, v, names)."""
    nd = info["node"]
    names = ["below", "above", "straddle", "straddle2", "equal"]
    a = np.array([nd[x] for x in names])
    M = np.full(len(a), nd["M"])
    return np.concatenate([a, M]).astype(np.int32), np.concatenate([M, a]).astype(np.int32), names + names


def merge_classes(A, info):
    """Where the entries of each merge row lie relative to M[C - 1] = info['last1'] -> {name: (entries <= last1, entries, holds
    last1)}: what the host test holds against the classes the cursor cases need."""
    out = {}
    for nm in ("below", "above", "straddle", "straddle2", "equal"):
        r = A.indices[A.indptr[info["node"][nm]]:A.indptr[info["node"][nm] + 1]]
        out[nm] = (int((r <= info["last1"]).sum()), len(r), bool((r == info["last1"]).any()))
    return out


def queue_chunks(info, Q):
    """64-pair chunks for the hit queue of the generic kernel (unit values, float32 weights) -> (u, v, hits): hits[c][j] = the
    common neighbours of pair j of chunk c, realised as (T, H) or (H, T); 0 = (Z, H): rows that are searched and share nothing."""
    k = queue_hit_counts(Q)
    fill = [k["slice"]] * (Q // 64 - 1)                     # brings the queue to Q - 64
    rest = lambda c: c + [0] * (64 - len(c))               # noqa: E731
    chunks = [
        rest(fill + [k["slice"], k["one"]]),                # a slice on Q - 64: no flush, the queue exactly full; the next pair flushes
        rest(fill + [k["one"], k["few"]]),                  # Q - 63 before a slice: a flush
        rest(fill + [k["open1"], k["few"]]),                # a pair open across one flush
        rest(fill + [k["open2"], k["one"]]),                # ... across two
        [0] * (64 - len(fill) - 1) + fill + [k["slice"]],   # the chunk ends with the queue exactly full
        rest([0, 0] + fill + [0, k["slice"], 0, k["few"], k["open2"], k["open1"]]),
    ]
    by_hits = {c: info["node"]["T_" + nm] for nm, c in k.items()}
    by_hits[0] = info["node"]["Z"]
    H = info["node"]["H"]
    u, v = [], []
    for ci, ch in enumerate(chunks):
        assert len(ch) == 64
        for j, c in enumerate(ch):
            a, b = by_hits[c], H
            if (ci + j) % 3 == 2:
                a, b = b, a
            u.append(a); v.append(b)
    return np.array(u, np.int32), np.array(v, np.int32), chunks


def queue_events(chunk_hits, Q):
    """The generic kernel's queue over one 64-pair chunk, given each pair's hits (a pair's slices of the shorter row hold 64 hits
    each, the last one the remainder; a slice without hits does not touch the queue) -> set of events:
    'slice_on_Q-64' (no flush), 'flush_on_Q-63', 'open_1' / 'open_2' (a pair open across that many flushes), 'pair_restarts_at_0'
    (a pair whose first slice flushes: it starts at slot 0), 'ends_full'."""
    ev, qlen = set(), 0
    for c in chunk_hits:
        flushes, first = 0, True
        while c > 0:
            s = min(c, 64)
            if qlen == Q - 64:
                ev.add("slice_on_Q-64")
            if qlen > Q - 64:
                if qlen == Q - 63:
                    ev.add("flush_on_Q-63")
                if first:
                    ev.add("pair_restarts_at_0")
                else:
                    flushes += 1
                qlen = 0
            qlen += s
            assert qlen <= Q
            c -= s
            first = False
        if flushes:
            ev.add("open_%d" % flushes)
    if qlen == Q:
        ev.add("ends_full")
    return ev


def small_flags(deg, u, v, S):
    du, dv = deg[np.asarray(u, np.int64)], deg[np.asarray(v, np.int64)]
    return (np.minimum(du, dv) > 0) & (np.maximum(du, dv) <= S)


def split_decision(deg, u, v, S, stride):
    """-> (the device-side decision for this list, small pairs per 64-pair chunk): the classifier counts the small pairs of every
    ``stride``-th chunk and the split launch runs when they are MORE than SPLIT_NUM / SPLIT_DEN of the sampled pairs."""
    small = small_flags(deg, u, v, S)
    n_chunks = (len(small) + 63) // 64
    per_chunk = np.array([int(small[c * 64:(c + 1) * 64].sum()) for c in range(n_chunks)])
    sampled = np.concatenate([np.arange(c * 64, min(len(small), (c + 1) * 64)) for c in range(0, n_chunks, stride)])
    return int(small[sampled].sum()) * SPLIT_DEN > len(sampled) * SPLIT_NUM, per_chunk


def split_lists(A, info, S, C, stride, seed=12):
    """Pair lists around the device-side choice between the split launch and the one-pair-per-wave body -> {name: (u, v)}.
    Small pairs join two rows of 1 .. S entries, long pairs a row beyond S (the hub left out) with any non-empty row."""
    rng = np.random.default_rng(seed)
    deg = np.diff(A.indptr)
    sp = np.array(info["specials"])
    small_rows, long_rows = sp[(deg[sp] > 0) & (deg[sp] <= S)], sp[deg[sp] > S]
    some = sp[deg[sp] > 0]
    empty = info["row"][0]

    def small(k):
        return rng.choice(small_rows, k), rng.choice(small_rows, k)

    def long_(k):
        a, b = rng.choice(long_rows, k), rng.choice(some, k)
        flip = rng.random(k) < 0.5
        return np.where(flip, b, a), np.where(flip, a, b)

    def mixed(flags):
        flags = np.asarray(flags, bool)
        su, sv = small(len(flags))
        lu, lv = long_(len(flags))
        return np.where(flags, su, lu), np.where(flags, sv, lv)

    def chunk_with(k_small, size=64):
        f = np.zeros(size, bool)
        f[rng.choice(size, k_small, replace=False)] = True
        return f

    lists = {}
    for i, nch in enumerate((1, 2, 4, 5, stride, stride + 1, 2 * stride + 1)):                # (a ragged last chunk; both decisions)
        lists["chunks_%d" % nch] = mixed(rng.random(64 * (nch - 1) + 37) < (0.8 if i % 2 else 0.4))
    nch = 2 * stride + 1
    sampled = np.repeat(np.arange(nch) % stride == 0, 64)[:64 * (nch - 1) + 37]
    lists["sampled_small_rest_long"] = mixed(sampled)
    lists["sampled_long_rest_small"] = mixed(~sampled)
    at = 64 * SPLIT_NUM // SPLIT_DEN + 1                                                     # the fewest small pairs of 64 that split
    lists["one_chunk_below"] = mixed(chunk_with(at - 1))
    lists["one_chunk_at"] = mixed(chunk_with(at))
    counts = np.concatenate([chunk_with(c) for c in (0, 1, 4, 5)])
    lists["counts_split"] = mixed(np.concatenate([np.ones(64, bool), counts]))
    lists["counts_whole"] = mixed(np.concatenate([np.zeros(64, bool), counts]))
    # small rows against an empty partner: not small pairs -- zeros, written by the launch of the longer pairs
    u, v = mixed(np.concatenate([np.ones(64, bool), chunk_with(40), chunk_with(3)]))
    for c in (1, 2):
        at_ = 64 * c + rng.choice(64, 12, replace=False)
        u[at_[:5]] = empty
        v[at_[5:10]] = empty
        u[at_[10:]] = v[at_[10:]] = empty
    lists["empty_partner"] = (u, v)
    return {k: (a.astype(np.int32), b.astype(np.int32)) for k, (a, b) in lists.items()}


# ---------------------------------------------------------------------------------------------------------- column-run kernel
def run_lengths():
    return [1, 63, 64, 65, 255, 256, 257]


def row_u_lengths():
    return [255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1535, 1536, 1537]


def grouped_graph(Q, n=None, seed=21):
    """-> (A, info) for the column-run kernel; the stored part lives in the low ids, ``n`` pads it with isolated nodes.
    info['row_u'][L]: a row of L entries inside E, the hub's entries; 'full' = a column holding all of E, 'none' = one holding
    none of it.  The node-0 family: columns 'v0' (holds node 0 and Z) and 'v1' (Z only); rows 'u_a' (0 and some of Z), 'u_b' (some
    of Z), 'u_c' (0 and ids outside Z), 'u_d' (ids outside Z).  'vq' / 'u_one' / 'u_full': a column, a row with one hit and a row of
    node 0 and Q - 1 hits -- after u_one the queue holds 1, the units of u_full bring it to exactly Q, then node 0 is appended.
    'plain': rows of ~20 entries that match among themselves; 'empty': a row without entries."""
    rng = np.random.default_rng(seed)
    assert Q % 256 == 0
    names = ["hub", "full", "none", "v0", "v1", "u_a", "u_b", "u_c", "u_d", "vq", "u_one", "u_full", "empty", "zero_row"]
    node = {nm: 1 + i for i, nm in enumerate(names)}        # (node 0 is a node like any other: it gets a plain row below)
    ru = {L: 1 + len(names) + i for i, L in enumerate(row_u_lengths())}
    p0 = 1 + len(names) + len(ru)
    n_plain = 3000
    e0 = p0 + n_plain                                       # E = [e0, e0 + HUB), Z = the 2 Q ids after it, then ids nobody's column holds
    z0 = e0 + HUB
    o0 = z0 + 2 * Q
    n_stored = o0 + 256
    n = n_stored if n is None else n
    assert n >= n_stored
    E = np.arange(e0, e0 + HUB)
    Z = np.arange(z0, z0 + 2 * Q)
    out = np.arange(o0, o0 + 256)
    perm = rng.permutation(E)
    rows = {node["hub"]: E, node["full"]: E, node["none"]: out[:64]}
    for L, i in ru.items():
        rows[i] = perm[:L]
    rows[node["v0"]] = np.concatenate([[0], Z[:300]])
    rows[node["v1"]] = Z[:300]
    rows[node["u_a"]] = np.concatenate([[0], Z[100:140], out[:7]])
    rows[node["u_b"]] = np.concatenate([Z[5:50], out[:7]])
    rows[node["u_c"]] = np.concatenate([[0], Z[300:340], out[:9]])
    rows[node["u_d"]] = np.concatenate([Z[300:340], out[:9]])
    rows[node["vq"]] = np.concatenate([[0], Z])
    rows[node["u_one"]] = Z[-1:]
    rows[node["u_full"]] = np.concatenate([[0], Z[:Q - 1]])
    rows[node["zero_row"]] = np.array([0])                  # node 0 is its only entry: the only common neighbour with v0 / vq
    plain = np.arange(p0, p0 + n_plain)
    draws = np.concatenate([rng.choice(perm[:200], (n_plain, 18)), rng.choice(Z[:300], (n_plain, 2)),
                            (rng.random((n_plain, 1)) >= 0.3) * rng.choice(Z[:300], (n_plain, 1))], 1)   # (0 = node 0, for a third)
    rows.update({int(i): d for i, d in zip(plain, draws)})
    rows[0] = draws[0]
    A = _assemble(n, rows, rng)
    info = dict(n=n, n_stored=n_stored, node=node, row_u=ru, plain=plain, E=(e0, e0 + HUB), Z=(z0, z0 + 2 * Q))
    return A, info


def grouped_queue_fill(A, info, Q):
    """The column-run kernel's queue over the pairs (u_one, vq), (u_full, vq) at the head of a run -> the queue length at the
    moment node 0 is appended for u_full (units of 256 entries of row u; a unit with hits flushes first when more than Q - 256
    are queued; the bit of node 0 is never set, so a unit does not count it)."""
    nd = info["node"]
    col = set(A.indices[A.indptr[nd["vq"]]:A.indptr[nd["vq"] + 1]].tolist()) - {0}
    qlen = 0
    for r in (nd["u_one"], nd["u_full"]):
        row = A.indices[A.indptr[r]:A.indptr[r + 1]]
        for k0 in range(0, len(row), 256):
            h = sum(int(w) in col for w in row[k0:k0 + 256])
            if h and qlen > Q - 256:
                qlen = 0
            qlen += h
    return qlen


def grouped_lists(A, info, K, seed=22):
    """Pair lists for the column-run kernel -> {name: (u, v)}."""
    rng = np.random.default_rng(seed)
    nd, plain = info["node"], info["plain"]
    pl = lambda k: rng.choice(plain, k)                                                     # noqa: E731
    lists = {}
    # runs of equal v of every length of run_lengths(), each on a column of its own, in ascending v
    cols = np.sort(rng.choice(plain, len(run_lengths()), replace=False))
    lists["runs"] = (np.concatenate([pl(L) for L in run_lengths()]), np.concatenate([np.full(L, c) for L, c in zip(run_lengths(), cols)]))
    # the rows of u against the column that holds all of them and the one that holds none; the empty row both ways
    us = np.array(list(info["row_u"].values()) + [nd["hub"], nd["empty"], 0])
    lists["row_u"] = (np.concatenate([us, us, pl(20), [nd["full"], nd["hub"]]]),
                      np.concatenate([np.full(len(us), nd["full"]), np.full(len(us), nd["none"]), np.full(20, nd["empty"]),
                                      [nd["empty"], nd["empty"]]]))
    # node 0 in every role, in runs of v0 / v1; then the queue that is exactly full when node 0 is appended
    fam = np.array([nd[x] for x in ("u_a", "u_b", "u_c", "u_d", "zero_row")] + [0])
    fam = np.concatenate([fam, pl(58)])
    lists["node0"] = (np.concatenate([fam, fam, [nd["u_one"], nd["u_full"]], pl(30), [0, nd["v0"]]]),
                      np.concatenate([np.full(64, nd["v0"]), np.full(64, nd["v1"]), np.full(32, nd["vq"]), [nd["u_a"], 0]]))
    # chunk edges: exactly K and K + 1 pairs; a run that crosses the K boundary
    for name, total in (("K", K), ("K+1", K + 1)):
        runs = np.sort(rng.choice(plain, 40, replace=False))
        v = np.sort(rng.choice(runs, total))
        lists[name] = (pl(total), v)
    v = np.concatenate([np.sort(rng.choice(plain[:100], K - 100)), np.full(200, plain[200]), np.sort(rng.choice(plain[300:400], 300))])
    lists["run_across_K"] = (pl(len(v)), v)
    k = 300
    lists["unsorted"] = (np.concatenate([pl(k - 6), us[-6:]]), rng.permutation(np.concatenate([pl(k - 20), np.full(20, nd["v0"])])))
    return {k_: (a.astype(np.int32), b.astype(np.int32)) for k_, (a, b) in lists.items()}


def hashed_graph(B, pad=4096, seed=23):
    """-> (A, info, (u, v, names)) with n = B + pad: for x in (0, 777) the ids x and x + B fall on the same bit of the hashed
    bitmap.  Rows 'lo' (x), 'hi' (x + B) and 'both', each with or without a true common neighbour c, scored against each other
    as row u and as column v: u 'hi' on v 'lo' is the false positive the verification must reject."""
    rng = np.random.default_rng(seed)
    n = B + pad
    rows, u, v, names = {}, [], [], []
    nid = 10
    c_ids = np.array([5000, 3001 + B])                      # true common neighbours: one below B, one above
    noise_u, noise_v = np.arange(6000, 6040), np.arange(7000, 7300)
    for x in (0, 777):
        fam = {}
        for kind, ids in (("lo", [x]), ("hi", [x + B]), ("both", [x, x + B])):
            for common in (False, True):
                for role, noise in (("u", noise_u), ("v", noise_v)):
                    rows[nid] = np.concatenate([ids, c_ids if common else [], noise]).astype(np.int64)
                    fam[(kind, common, role)] = nid
                    nid += 1
        for (ku, cu, ru_), iu in fam.items():
            for (kv, cv, rv), iv in fam.items():
                if ru_ == "u" and rv == "v":
                    u.append(iu); v.append(iv)
                    names.append((x, ku, cu, kv, cv))
    A = _assemble(n, rows, rng)
    order = np.argsort(np.array(v), kind="stable")          # runs of equal v
    u, v = np.array(u, np.int32)[order], np.array(v, np.int32)[order]
    return A, dict(n=n), (u, v, [names[i] for i in order])
