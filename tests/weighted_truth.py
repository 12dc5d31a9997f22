"""Host truth of the stored-value (weighted) scoring path, in plain numpy: no GPU, no kernel of the package.

A graph with stored values scores a two-hop non-edge {u, v} by  sum_w (A[u,w] * A[v,w]) * node_w[w].  The fused expansion
(csrc/expand_score.hip), the weighted re-scoring (csrc/rescore.hip) and through it scan_topk all define that sum the same way:
every path's term is formed in float32 -- t = fl(fl(a_u * a_v) * w): two multiplies, no add, so nothing can be contracted --,
converted to 2^-40 fixed point with round-half-even, the terms are summed in int64 (any order: exact) and the score is
float32(float64(sum) x 2^-40).  ``exact_scores`` states exactly that; ``real_scores`` is the same sum without any rounding
(float64 products of the float32 inputs), which the bounds of the screening scores are stated against.

The suite's older weighted graphs draw their values from small integers, whose float32 products are exact; the value families
below (``FAMILIES``) make every product round, spread the magnitudes over twenty binades, shrink the values to 2^-12 .. 2^-10
(terms around 2^-22: the scores then use few bits of the screening word; a term below half a fixed-point unit needs a weight
below 2^-19, which none of the tables holds -- the ties of that rounding are held by the host test alone), or lift the scores
into the high bits of the scan's 31-bit screening word.

tests/test_weighted_truth_host.py holds this file to a triple Python loop on the CPU; tests/test_gpu_weighted_values.py holds the
kernels to it."""
import numpy as np

FIX = 40                          # the exact scores' fixed point: units of 2^-40
EXACT_LIMIT = 1 << 53             # int64 sums below this convert to float64 exactly
FUSED_SCORE_LIMIT = float(1 << 22)    # candidates.FUSED_SCORE_LIMIT: what the fused kernels' accumulators are allowed
GRAPHS = ("rmat11", "er300")
FAMILIES = ("ints", "mantissa", "wide", "tiny", "big_scores")
TABLES = ("aa", "ra", "ones", "aa_zeroed")
ZERO_EVERY = 7                    # table aa_zeroed: nodes 0, 7, 14, ... weigh nothing (candidates of score 0)
W_AA, W_RA = 0, 1                 # (the oracle's mode numbers)
BIG_BOUND = 4096.0                # big_scores: the score bound under unit node weights (sums stay below 2^53 units of 2^-40)

# Combinations that the scan refuses -- scan.scan_usable is False for each, for the reason given -- and that are therefore no
# case of the GPU tests (tests/test_weighted_truth_host.py checks that each reason is true and that every other combination has
# non-negative weights, a score bound below FUSED_SCORE_LIMIT and exact sums below 2^53).
NEGATIVE_AA = "an Adamic-Adar weight 1 / log(value sum) is negative where a node's stored values sum to less than 1"
BEYOND_RANGE = "products of values up to 2^11 put the score bound beyond the fused kernels' fixed-point range (2^22)"
BEYOND_EXACT = "scores of 2^13 and more: the int64 sums leave the 2^53 units of 2^-40 that float64 holds exactly"
REMOVED = {}
for _f in ("mantissa", "wide", "tiny", "big_scores"):            # (big_scores scales this graph's values DOWN: its hubs set the bound)
    for _t in ("aa", "aa_zeroed"):
        REMOVED[("rmat11", _f, _t)] = NEGATIVE_AA
for _t in ("aa", "aa_zeroed"):
    REMOVED[("er300", "tiny", _t)] = NEGATIVE_AA
    REMOVED[("er300", "wide", _t)] = BEYOND_EXACT
for _g in GRAPHS:
    REMOVED[(_g, "wide", "ones")] = BEYOND_RANGE


def cases():
    """Every (graph, family, table) the GPU tests run."""
    return [(g, f, t) for g in GRAPHS for f in FAMILIES for t in TABLES if (g, f, t) not in REMOVED]


class Graph:
    """A symmetric CSR graph with one float32 value per undirected edge (mirror entries equal), no diagonal, rows sorted."""

    def __init__(self, n, lo, hi, val):
        lo, hi, val = np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.asarray(val, np.float32)
        assert (lo < hi).all() and len(np.unique(hi * n + lo)) == len(lo) and (val > 0).all()
        r, c, a = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([val, val])
        o = np.argsort(r * n + c, kind="stable")
        self.n, self.col, self.val = int(n), c[o], a[o]
        self.rowptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=n), out=self.rowptr[1:])
        self.lo, self.hi, self.edge_val = lo, hi, val

    @property
    def nnz(self):
        return len(self.col)

    def degree(self):
        return np.diff(self.rowptr)

    def row_index(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), self.degree())

    def with_values(self, val):
        return Graph(self.n, self.lo, self.hi, val)


def edges_of(n, r, c):
    """The distinct undirected edges (lo < hi) among the pairs (r, c); loops dropped."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    keep = r != c
    lo, hi = np.minimum(r, c)[keep], np.maximum(r, c)[keep]
    key = np.unique(hi * n + lo)
    return key % n, key // n


def patterns(synth):
    """name -> (n, lo, hi): the R-MAT of scale 11 (as generated: low ids are the hubs, several with hundreds of neighbours) and
    an Erdos-Renyi graph of 300 nodes whose longest row stays below the 64 lanes of a wave."""
    out = {}
    ei = synth.rmat_edges(11, 10 << 11, 8, "cpu").numpy()
    out["rmat11"] = (1 << 11,) + edges_of(1 << 11, ei[0], ei[1])
    rng = np.random.default_rng(300)
    iu, ju = np.triu_indices(300, 1)
    pick = rng.random(len(iu)) < 0.05
    out["er300"] = (300, iu[pick].astype(np.int64), ju[pick].astype(np.int64))
    return out


def _seed(name, family):
    return [GRAPHS.index(name), FAMILIES.index(family), 20261]


def family_values(name, family, n, lo, hi):
    """float32 values of the undirected edges (lo, hi) of graph ``name`` under a value family (seeded)."""
    return draw_values(family, np.random.default_rng(_seed(name, family)), n, lo, hi)


def draw_values(family, rng, n, lo, hi):
    m = len(lo)
    if family == "ints":
        return rng.integers(1, 6, m).astype(np.float32)
    if family == "mantissa":
        return np.exp(rng.standard_normal(m)).astype(np.float32)
    if family == "wide":
        return (2.0 ** rng.integers(-10, 11, m) * (1.0 + rng.random(m))).astype(np.float32)
    if family == "tiny":
        return rng.uniform(2.0 ** -12, 2.0 ** -10, m).astype(np.float32)
    assert family == "big_scores"
    return _big_scores(n, lo, hi, np.exp(rng.standard_normal(m)), rng)


def _big_scores(n, lo, hi, val, rng):
    """``mantissa`` values, lifted so that the graph's best score lies within a factor of 4 of its score bound
    (candidates.fused_score_bound: max_v sum_w A[v,w] node_w[w] max_u A[u,w]) and scaled so that this bound is BIG_BOUND under
    unit node weights.  A uniform scale moves the best score and the bound alike, so the edges of ONE candidate pair -- the one
    with the most common neighbours that table aa_zeroed leaves a weight -- to its common neighbours are made to dominate the
    rows of both ends: 64 x U[1, 2) against values around 1.  The scan then picks the shift that puts the bound into bits 30 / 31
    of the screening word, and that pair's screening sum lies within two bits of it."""
    g = Graph(n, lo, hi, np.ones(len(lo), np.float32))
    pu, pw, pv, _, _ = paths(g.rowptr, g.col)
    ok = pw % ZERO_EVERY != 0
    key, cnt = np.unique(pv[ok] * n + pu[ok], return_counts=True)
    best = key[np.argmax(cnt)]
    u, v = int(best % n), int(best // n)
    common = pw[ok & (pu == u) & (pv == v)]
    val = val.copy()
    for x in (u, v):
        a, b = np.minimum(x, common), np.maximum(x, common)
        at = np.flatnonzero(np.isin(hi * n + lo, b * n + a))
        assert len(at) == len(common)
        val[at] = 64.0 * (1.0 + rng.random(len(at)))
    g = g.with_values(val.astype(np.float32))
    scale = np.sqrt(BIG_BOUND / bound_formula(g, np.ones(n, np.float32)))
    return (val * scale).astype(np.float32)


def graphs(synth):
    """(graph name, family) -> Graph, for every graph and family."""
    out = {}
    for name, (n, lo, hi) in patterns(synth).items():
        for family in FAMILIES:
            out[(name, family)] = Graph(n, lo, hi, family_values(name, family, n, lo, hi))
    return out


def node_table(oracle, g, table):
    """float32[N] node weights of ``g``: Adamic-Adar / resource allocation from the oracle's float32 value sums, ones, or the
    Adamic-Adar table with every ZERO_EVERY-th node's weight set to 0."""
    if table == "ones":
        return np.ones(g.n, np.float32)
    cs = oracle.col_sums(g.rowptr, g.col.astype(np.int32), g.val, g.n)
    w = oracle.node_weights(cs, W_RA if table == "ra" else W_AA).astype(np.float32)
    if table == "aa_zeroed":
        w[::ZERO_EVERY] = 0.0
    return w


def is_edge(rowptr, col, u, v):
    """Whether (u[i], v[i]) is a stored entry, for arrays of pairs."""
    n = len(rowptr) - 1
    key = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + np.asarray(col, np.int64)      # (ascending in CSR order)
    want = np.asarray(u, np.int64) * n + np.asarray(v, np.int64)
    at = np.minimum(np.searchsorted(key, want), max(len(key) - 1, 0))
    return key[at] == want if len(key) else np.zeros(len(want), bool)


def paths(rowptr, col):
    """Every two-hop path u - w - v with u < v and (u, v) not an edge: (u, w, v, eu, ev) as int64 arrays, eu / ev the stored
    entries (w, u) / (w, v) of row w -- whose values are A[u,w] / A[v,w] on a symmetric graph.  Rows are sorted, so the paths
    through w are the pairs (i < j) of positions of its row."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, nnz = len(rowptr) - 1, len(col)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    pos = np.arange(nnz, dtype=np.int64) - rowptr[row]                 # entry j of a row pairs with the j entries before it
    first = np.zeros(nnz + 1, np.int64)
    np.cumsum(pos, out=first[1:])
    ev = np.repeat(np.arange(nnz, dtype=np.int64), pos)
    eu = rowptr[row[ev]] + (np.arange(first[-1], dtype=np.int64) - first[ev])
    u, v, w = col[eu], col[ev], row[ev]
    keep = ~is_edge(rowptr, col, u, v)
    return u[keep], w[keep], v[keep], eu[keep], ev[keep]


def _grouped(n, u, v):
    """Sort order of the paths by pair key, the distinct keys (v << 32 | u, ascending) and where each pair's run starts."""
    key = (v << 32) | u
    o = np.argsort(key, kind="stable")
    keys, start, count = np.unique(key[o], return_index=True, return_counts=True)
    return o, keys, start, count


def fixed_term(a_u, a_v, w):
    """int64 2^-40 fixed-point value of a path's float32 term fl(fl(a_u * a_v) * w) (rint: half to even, like __double2ll_rn)."""
    t = (np.asarray(a_u, np.float32) * np.asarray(a_v, np.float32)).astype(np.float32) * np.asarray(w, np.float32)
    assert t.dtype == np.float32
    return np.rint(t.astype(np.float64) * 2.0 ** FIX).astype(np.int64)


def exact_scores(rowptr, col, val, node_w, the_paths=None):
    """(keys int64 ascending: v << 32 | u, sums int64 in units of 2^-40, scores float32, path counts int64) of every candidate."""
    u, w, v, eu, ev = paths(rowptr, col) if the_paths is None else the_paths
    val, node_w = np.asarray(val, np.float32), np.asarray(node_w, np.float32)
    q = fixed_term(val[eu], val[ev], node_w[w])
    o, keys, start, count = _grouped(len(rowptr) - 1, u, v)
    if not len(keys):
        return keys, np.zeros(0, np.int64), np.zeros(0, np.float32), count
    # (a bound that holds whatever the signs, so that the int64 sums below cannot have wrapped either)
    assert float(np.add.reduceat(np.abs(q[o]).astype(np.float64), start).max()) < EXACT_LIMIT, "a sum of 2^53 units or more"
    sums = np.add.reduceat(q[o], start)
    return keys, sums, (sums.astype(np.float64) * 2.0 ** -FIX).astype(np.float32), count


def real_scores(rowptr, col, val, node_w, the_paths=None):
    """float64 scores of the same candidates (same order as exact_scores' keys) from unrounded products."""
    u, w, v, eu, ev = paths(rowptr, col) if the_paths is None else the_paths
    val, node_w = np.asarray(val, np.float64), np.asarray(node_w, np.float64)
    t = val[eu] * val[ev] * node_w[w]
    o, keys, start, _ = _grouped(len(rowptr) - 1, u, v)
    return np.add.reduceat(t[o], start) if len(keys) else np.zeros(0)


def pair_exact(rowptr, col, val, node_w, u, v):
    """The same definition for ONE arbitrary pair (an edge, u == v, no common neighbour ...): float32 score."""
    ub, ue, vb, ve = rowptr[u], rowptr[u + 1], rowptr[v], rowptr[v + 1]
    _, iu, iv = np.intersect1d(col[ub:ue], col[vb:ve], assume_unique=True, return_indices=True)
    q = fixed_term(val[ub:ue][iu], val[vb:ve][iv], np.asarray(node_w, np.float32)[col[ub:ue][iu]])
    return np.float32(float(int(q.sum())) * 2.0 ** -FIX)


def bound_formula(g, node_w):
    """max_v sum_w |A[v,w]| |node_w[w]| max_u |A[u,w]| in float64: the docstring of candidates.fused_score_bound."""
    colmax = np.zeros(g.n, np.float64)
    np.maximum.at(colmax, g.col, np.abs(g.val.astype(np.float64)))
    term = np.abs(g.val.astype(np.float64)) * np.abs(np.asarray(node_w, np.float64))[g.col] * colmax[g.col]
    rows = np.zeros(g.n, np.float64)
    np.add.at(rows, g.row_index(), term)
    return float(rows.max()) if g.n else 0.0


class Truth:
    """Everything the GPU tests compare one (graph, family, table) with."""

    def __init__(self, g, node_w, the_paths):
        self.g, self.node_w = g, np.asarray(node_w, np.float32)
        self.keys, self.sums, self.scores, self.counts = exact_scores(g.rowptr, g.col, g.val, self.node_w, the_paths)
        self.real = real_scores(g.rowptr, g.col, g.val, self.node_w, the_paths)
        self.u, self.v = self.keys & 0xFFFFFFFF, self.keys >> 32
        self.exact64 = self.sums.astype(np.float64) * 2.0 ** -FIX

    def at(self, keys):
        """Positions of ``keys`` in the truth's key list; every one must be a candidate."""
        at = np.searchsorted(self.keys, keys)
        assert (at < len(self.keys)).all() and np.array_equal(self.keys[np.minimum(at, len(self.keys) - 1)], keys), "not a candidate"
        return at
