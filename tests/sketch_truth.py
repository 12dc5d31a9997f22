"""The truth the subgraph sketches (csrc/sketch.hip, ops.sketch_*, CSRGraph.sketches, heuristics.sketch_*) are held to: a numpy
restatement of DESIGN 4.5h.  The sketches are integer arithmetic only (uint64 products wrap mod 2^64; ranks from integer bit
lengths, no logarithm), so the HIP tables and statistics must equal these bit for bit.  A plain helper module (no fixtures);
tests/test_sketch_host.py validates it on the CPU against sketches built from explicit sets and against exact counts.

A graph is a scipy CSR matrix with sorted indices; only its PATTERN counts."""
import numpy as np
import scipy.sparse as ssp
import torch

import training_truth as tt

R, P = 256, 128                      # HyperLogLog registers (bytes), MinHash words (uint32)
MAX_RANK = 33
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix64(x):
    """The splitmix64 finaliser on a uint64 array (or int), mod 2^64."""
    z = np.atleast_1d(np.asarray(x, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def bit_length32(w):
    """Bits needed for each uint32 of ``w`` (0 for 0), by shifts and compares."""
    t = np.asarray(w, dtype=np.uint64).copy()
    bl = np.zeros(t.shape, np.int64)
    for s in (16, 8, 4, 2, 1):
        m = (t >> np.uint64(s)) > 0
        bl += m * s
        t = np.where(m, t >> np.uint64(s), t)
    return bl + (t > 0)


def own_register(ids):
    """-> (idx, rank) of the one non-zero HyperLogLog register of each id."""
    h = mix64(ids)
    idx = (h >> np.uint64(56)).astype(np.int64)
    w = (h >> np.uint64(24)) & np.uint64(0xFFFFFFFF)
    rank = np.where(w == 0, MAX_RANK, 32 - bit_length32(w) + 1)
    return idx, rank.astype(np.int64)


def own_sketch(ids):
    """-> (hll uint8 [n, 256], mh uint32 [n, 128]) of the ids (0 <= id < 2^31)."""
    ids = np.atleast_1d(np.asarray(ids, dtype=np.uint64))
    idx, rank = own_register(ids)
    hll = np.zeros((len(ids), R), np.uint8)
    hll[np.arange(len(ids)), idx] = rank
    salt = (np.arange(1, P + 1, dtype=np.uint64) << np.uint64(32))[None, :]
    mh = (mix64(ids[:, None] ^ salt) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(len(ids), P)
    return hll, mh


def empty_sketch(n=1):
    return np.zeros((n, R), np.uint8), np.full((n, P), 0xFFFFFFFF, np.uint32)


def sketch_of_set(members):
    """The sketch of an explicit set of node ids: the union of its members' own sketches."""
    members = np.asarray(sorted(members), dtype=np.uint64)
    if len(members) == 0:
        h, m = empty_sketch()
        return h[0], m[0]
    h, m = own_sketch(members)
    return h.max(0), m.min(0)


def _csr(A):
    A = ssp.csr_matrix(A)
    A.sort_indices()
    return A


def propagate(A, hll, mh, keep_own):
    """out[v] = the union of in[w] over the stored entries w of row v, with ``keep_own`` also of in[v]."""
    A = _csr(A)
    out_h, out_m = empty_sketch(A.shape[0])
    for v in range(A.shape[0]):
        w = A.indices[A.indptr[v]:A.indptr[v + 1]]
        if keep_own:
            w = np.concatenate([w, [v]])
        if len(w):
            out_h[v], out_m[v] = hll[w].max(0), mh[w].min(0)
    return out_h, out_m


def tables(A, hops=2):
    """-> (hll uint8 [hops, n, 256], mh uint32 [hops, n, 128]): own -> hop 1 (keep_own = 0) -> hop 2 (keep_own = 1, from hop 1)."""
    n = A.shape[0]
    tabs = [propagate(A, *own_sketch(np.arange(n)), keep_own=False)]
    if hops == 2:
        tabs.append(propagate(A, *tabs[0], keep_own=True))
    return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])


def exact_sets(A, hops=2):
    """[S_1, S_2] as boolean scipy CSR matrices: S_1(v) = N(v), S_2(v) = S_1(v) with the S_1 of every stored neighbour."""
    Pm = _csr(A).copy()
    Pm.data = np.ones(len(Pm.data), np.int64)
    sets = [Pm.astype(bool).tocsr()]
    if hops == 2:
        sets.append((Pm + Pm @ Pm).astype(bool).tocsr())
    return sets


def pair_stats(hll, mh, u, v):
    """-> (S int64, Z int64, match int64), each [B, K, K]; a pair with an id outside [0, n) holds -1 everywhere."""
    K, n = hll.shape[0], hll.shape[1]
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    ok = (u >= 0) & (u < n) & (v >= 0) & (v < n)
    uc, vc = np.where(ok, u, 0), np.where(ok, v, 0)
    S = np.full((len(u), K, K), -1, np.int64)
    Z, M = S.copy(), S.copy()
    for i in range(K):
        for j in range(K):
            mx = np.maximum(hll[i][uc], hll[j][vc]).astype(np.int64)
            term = np.where(mx <= MAX_RANK, np.int64(1) << np.clip(MAX_RANK - mx, 0, 62), 0)
            S[:, i, j] = np.where(ok, term.sum(1), -1)
            Z[:, i, j] = np.where(ok, (mx == 0).sum(1), -1)
            M[:, i, j] = np.where(ok, (mh[i][uc] == mh[j][vc]).sum(1), -1)
    return S, Z, M


def cardinality(S, Z):
    """The HyperLogLog estimate (float64) from the integers; linear counting below 2.5 m; the empty set gives 0."""
    m = 256.0
    alpha = 0.7213 / (1.0 + 1.079 / m)
    S, Z = np.asarray(S, np.float64), np.asarray(Z, np.int64)
    e = (alpha * m * m * 8589934592.0) / S
    lin = m * np.log(m / np.maximum(Z, 1))
    return np.where((e <= 2.5 * m) & (Z > 0), lin, e)


def row_cardinality(hll):
    """C [K, n]: the estimate of every row of the tables."""
    h = hll.astype(np.int64)
    return cardinality((np.int64(1) << (MAX_RANK - h)).sum(-1), (h == 0).sum(-1))


def intersections(S, Z, match):
    return (np.asarray(match, np.float64) / 128.0) * cardinality(S, Z)


def features(I, cu, cv):
    """The structural features in numpy float64, each in the written association, rounded once to float32: I [B, K, K], cu / cv
    [K, B] the cardinalities C_k of the two endpoints -> [B, 5] (K = 2) or [B, 2] (K = 1)."""
    I, cu, cv = np.asarray(I, np.float64), np.asarray(cu, np.float64), np.asarray(cv, np.float64)
    i11 = I[:, 0, 0]
    if I.shape[1] == 1:
        cols = [i11, (cu[0] - i11) + (cv[0] - i11)]
    else:
        i12, i21, i22 = I[:, 0, 1], I[:, 1, 0], I[:, 1, 1]
        a12 = (i12 - i11) + (i21 - i11)
        a22 = (i22 - (i12 + i21)) + i11
        b1 = (cu[0] - i12) + (cv[0] - i21)
        b2 = (((cu[1] - cu[0]) - i22) + i12) + (((cv[1] - cv[0]) - i22) + i21)
        cols = [i11, a12, a22, b1, b2]
    return np.log1p(np.maximum(np.stack(cols, 1), 0.0)).astype(np.float32)


def pair_features(hll, mh, u, v):
    """-> (I float64 [B, K, K], F float32 [B, 5 | 2]) of the pairs from the tables, everything above in numpy."""
    I = intersections(*pair_stats(hll, mh, u, v))
    C = row_cardinality(hll)
    return I, features(I, C[:, np.asarray(u, np.int64)], C[:, np.asarray(v, np.int64)])


def buddy_forward(p, A, x, edges, feats, hops, branch=None, pre=None):
    """BuddyLinkModel in training mode with dropout 0 (which is also its eval forward) -> scores [B], dense torch in the dtype of
    ``A``: xin = [emb.weight || x] (embedding first), h = feat_lin([xin || An xin || ... || An^hops xin]) with An GCNConv's
    normalised aggregate of the dense adjacency ``A``, t = relu(xij_lin(h_u * h_v)) + relu(xs_lin(F)), relu(lin(t)) for
    lins[:-1], sigmoid(lins[-1](t)).  ``feats``: the pairs' structural features (constants).  ``branch`` / ``pre``: see
    ``training_truth._relu`` (forward order: xij_lin, xs_lin, lins[:-1])."""
    branch = None if branch is None else iter(branch)
    dt = A.dtype
    xin = x.to(dt) if "emb.weight" not in p else (p["emb.weight"] if x is None else torch.cat([p["emb.weight"], x.to(dt)], 1))
    An = tt.gcn_matrix(A)
    xs = [xin]
    for _ in range(hops):
        xs.append(An @ xs[-1])
    h = torch.cat(xs, 1) @ p["feat_lin.weight"].t() + p["feat_lin.bias"]
    zij = tt._relu((h[edges[0]] * h[edges[1]]) @ p["linkpred.xij_lin.weight"].t() + p["linkpred.xij_lin.bias"], branch, pre)
    zs = tt._relu(feats.to(dt) @ p["linkpred.xs_lin.weight"].t() + p["linkpred.xs_lin.bias"], branch, pre)
    t = zij + zs
    M = tt._count(p, "linkpred.lins.{}.weight")
    for i in range(M - 1):
        t = tt._relu(t @ p[f"linkpred.lins.{i}.weight"].t() + p[f"linkpred.lins.{i}.bias"], branch, pre)
    return torch.sigmoid(t @ p[f"linkpred.lins.{M - 1}.weight"].t() + p[f"linkpred.lins.{M - 1}.bias"]).squeeze(1)


def exact_intersections(sets, u, v):
    """|S_i(u) & S_j(v)| [B, K, K] from the explicit sets."""
    K = len(sets)
    out = np.zeros((len(u), K, K), np.int64)
    for i in range(K):
        for j in range(K):
            out[:, i, j] = np.asarray(sets[i][u].multiply(sets[j][v]).sum(1)).ravel()
    return out


# ---------------------------------------------------------------------------------------------------------- graphs
def _rows_to_csr(rows, n):
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    idx = np.concatenate([np.asarray(r, np.int64) for r in rows]) if n else np.zeros(0, np.int64)
    return ssp.csr_matrix((np.ones(len(idx), np.float32), idx.astype(np.int32), indptr), shape=(n, n))


LONGEST_ROW = 11                     # boundary_graph: the row of 3 rc + 2 entries that spans five pieces
BOUNDARY_CLASSES = ("0", "1", "rc-1", "rc", "rc+1", "2rc+1")


def boundary_lengths(rc):
    return dict(zip(BOUNDARY_CLASSES, (0, 1, rc - 1, rc, rc + 1, 2 * rc + 1)))


def boundary_graph(rc, seed=5):
    """A directed graph for eps_sketch_propagate's paths, ``rc`` = its row chunk: rows of 0, 1, rc - 1, rc, rc + 1 and 2 rc + 1
    entries; row 0 (rc entries, a stored self loop) makes row 1 (2 rc + 1) begin exactly on a cut and row 2 (rc + 1) begin inside
    the piece that holds row 1's tail; two more long rows follow each other further on; row 10 (rc - 8 entries) puts row 11
    (``LONGEST_ROW``: 3 rc + 2 entries) on the last entry of a piece, so that it spans FIVE pieces -- more partial slots than one
    trip of the kernel's combine loop takes; the last node has no row and is only ever a neighbour; n is odd.
    -> (scipy CSR, {class: [rows]})."""
    rng = np.random.default_rng(seed)
    n = max(2 * rc + 519, 3 * rc + 5)
    n += 1 - n % 2
    last = n - 1

    def pick(k, must=()):
        pool = np.setdiff1d(np.arange(n - 1), np.asarray(must, np.int64))
        got = rng.choice(pool, size=k - len(must), replace=False)
        return np.sort(np.concatenate([got, np.asarray(must, np.int64)]))

    lens = {0: rc, 1: 2 * rc + 1, 2: rc + 1, 3: 0, 4: 1, 5: rc - 1, 6: 3, 7: rc + 1, 8: 2 * rc + 1, 9: rc, 10: rc - 8,
            LONGEST_ROW: 3 * rc + 2}
    rows = []
    for v in range(n):
        if v in lens:
            k = lens[v]
            rows.append(pick(k, (0,) if v == 0 else (last,) if v == 4 else ()) if k else np.zeros(0, np.int64))
        elif v == last or v % 7 == 3:
            rows.append(np.zeros(0, np.int64))
        else:
            rows.append(pick(int(rng.integers(1, 24))))
    A = _rows_to_csr(rows, n)
    deg = np.diff(A.indptr)
    return A, {c: np.flatnonzero(deg == k).tolist() for c, k in boundary_lengths(rc).items()}


def skewed_graph(n=3000, m=24000, seed=11):
    """A symmetric graph with a heavy-tailed degree sequence (endpoint i drawn with weight (i + 1)^-0.9), no self loops: the
    accuracy fixture of the estimator."""
    rng = np.random.default_rng(seed)
    w = (np.arange(n) + 1.0) ** -0.9
    w /= w.sum()
    a, b = rng.choice(n, m, p=w), rng.choice(n, m, p=w)
    keep = a != b
    a, b = a[keep], b[keep]
    A = ssp.coo_matrix((np.ones(2 * len(a), np.float32), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    return A


def accuracy(A, n_pairs=4000, seed=3):
    """-> dict: Pearson correlation of I_11, I_12, I_22 with the exact counts over uniformly drawn pairs, and the mean relative
    error of C_1, C_2 over the nodes with a non-empty set."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    u, v = rng.integers(0, n, n_pairs), rng.integers(0, n, n_pairs)
    hll, mh = tables(A, 2)
    est = intersections(*pair_stats(hll, mh, u, v))
    sets = exact_sets(A, 2)
    exact = exact_intersections(sets, u, v)
    out = {}
    for name, (i, j) in {"I11": (0, 0), "I12": (0, 1), "I22": (1, 1)}.items():
        out[name] = float(np.corrcoef(est[:, i, j], exact[:, i, j])[0, 1])
    C = row_cardinality(hll)
    for k in range(2):
        size = np.asarray(sets[k].sum(1)).ravel().astype(np.float64)
        nz = size > 0
        out[f"C{k + 1}"] = float((np.abs(C[k][nz] - size[nz]) / size[nz]).mean())
    return out
