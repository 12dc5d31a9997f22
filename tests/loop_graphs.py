"""Small symmetric graphs WITH stored self loops, their loop-free twins, and the host truths the GPU tests of the filter step
are held to on them (tests/test_gpu_self_loops.py; tests/test_loop_graphs_host.py pins, from the oracle alone, the conditions
that keep those tests from passing vacuously).  scipy and numpy only: no GPU, no import of the package.

What the right answer is follows from filter.py:96-109 (A @ A, minus the diagonal, minus the known edges): a stored loop never
makes or removes a candidate (u in N(u) is a common neighbour of (u, v) only if u in N(v), and then (u, v) is an edge), but it
counts in the column sums, so the AA / RA weight of its node -- and with it the scores -- move.

Every truth is built from oracle.candidates_scipy(_columns), col_sums, node_weights, pair_scores and pair_scores_f64, the way
tests/test_gpu_scan.py::_oracle_candidates builds its own."""
import os
from collections import namedtuple

import numpy as np
import scipy.sparse as ssp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

K_INSIDE = {"rmat_loops": 1000, "collab_like_loops": 777}          # a K well inside the candidate set of each graph
HUBS = 3                                                           # the highest-degree nodes that are looped on purpose
STRUCTURED = ("star", "path", "two_cliques", "complete")
WIDE_NODES = 600_000                                               # past the 589 824 ids the two-pass scan takes in ONE id window

LoopGraph = namedtuple("LoopGraph", "name A twin weighted loop_alone loop_plus_one hubs")
Truth = namedtuple("Truth", "pairs count cn f32 f64 weights")
_GRAPHS, _TRUTHS = {}, {}


def _csr(A):
    A = A.tocsr().astype(np.float32)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def _sym_unit(n, r, c):
    A = ssp.coo_matrix((np.ones(len(r), np.float32), (r, c)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float32).tocsr()
    A.setdiag(0)
    return _csr(A)


def with_loops(A, nodes, values=None):
    """A plus the diagonal entries of ``nodes`` (values 1, or ``values``); A itself has an empty diagonal."""
    nodes = np.unique(np.asarray(nodes, np.int64))
    vals = np.ones(len(nodes), np.float32) if values is None else np.asarray(values, np.float32)
    assert A.diagonal().sum() == 0 and len(vals) == len(nodes) and (vals > 0).all()
    return _csr(A + ssp.coo_matrix((vals, (nodes, nodes)), shape=A.shape).tocsr())


def without_loops(A):
    B = A.tolil(copy=True)
    B.setdiag(0)
    return _csr(B.tocsr())


def looped_nodes(A):
    return np.flatnonzero(A.diagonal() != 0)


def _placements(twin, rng, share=1 / 3):
    """The looped nodes of a graph: a third of all, the HUBS highest-degree nodes (hub rows / head rows under hubs-first labels),
    five nodes without a neighbour, five with exactly one, the lowest and the highest id.
    -> (nodes, the loop-alone ones, the loop-plus-one ones, the hubs)."""
    n = twin.shape[0]
    deg = np.diff(twin.indptr)
    hubs = np.argsort(-deg, kind="stable")[:HUBS]
    alone, plus_one = np.flatnonzero(deg == 0)[:5], np.flatnonzero(deg == 1)[:5]
    assert len(alone) == 5 and len(plus_one) == 5, "the graph has too few nodes of degree 0 / 1 for the placements"
    nodes = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < share), hubs, alone, plus_one, [0, n - 1]]))
    return nodes, alone, plus_one, hubs


def _rmat_edges(rng, scale, m, a=0.45, b=0.22, c=0.22):
    r, col = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for _ in range(scale):
        q = rng.random(m)
        r = (r << 1) | (q >= a + b)
        col = (col << 1) | (((q >= a) & (q < a + b)) | (q >= a + b + c))
    return r, col


def _rmat_loops():
    """2060 nodes, unit: an R-MAT core of 2048 ids (scale 11, 4 edges per node), three planted hubs of degree about n / 5, six
    nodes without a neighbour and six with one, under a random relabelling; loops on a third of the nodes + the placements."""
    rng = np.random.default_rng(20)
    core, n = 2048, 2060
    r, c = _rmat_edges(rng, 11, 4 * core)
    hubs = rng.choice(core, HUBS, replace=False)
    r = np.concatenate([r, np.repeat(hubs, n // 5), np.arange(core + 6, n)])
    c = np.concatenate([c, rng.integers(0, core, HUBS * (n // 5)), rng.integers(0, core, n - core - 6)])
    perm = rng.permutation(n)
    twin = _sym_unit(n, perm[r], perm[c])
    nodes, alone, plus_one, top = _placements(twin, rng)
    return LoopGraph("rmat_loops", with_loops(twin, nodes), twin, False, alone, plus_one, top)


def _collab_like_loops():
    """tests/golden/pairs_collab_like.npz (512 nodes, summed integer multi-edge weights) with loops of value 2 .. 6: what
    to_symmetric leaves of (u, u) rows of weight 1 .. 3 -- the doubled diagonal."""
    d = np.load(os.path.join(GOLDEN, "pairs_collab_like.npz"))
    n = len(d["rowptr"]) - 1
    twin = _csr(ssp.csr_matrix((d["val"], d["col"], d["rowptr"]), shape=(n, n)))
    assert twin.diagonal().sum() == 0
    rng = np.random.default_rng(21)
    nodes, alone, plus_one, top = _placements(twin, rng)
    A = with_loops(twin, nodes, rng.integers(2, 7, len(nodes)))
    return LoopGraph("collab_like_loops", A, twin, True, alone, plus_one, top)


def _structured(name):
    rng = np.random.default_rng(22)
    if name == "star":                                # a hub of degree n - 1: loop on the hub and on some leaves
        n = 601
        twin = _sym_unit(n, np.zeros(n - 1, np.int64), np.arange(1, n))
        nodes = np.concatenate([[0, 1, n - 1], rng.choice(np.arange(2, n - 1), 150, replace=False)])
    elif name == "path":
        n = 1000
        twin = _sym_unit(n, np.arange(n - 1), np.arange(1, n))
        nodes = np.concatenate([[0, n - 1], np.arange(3, n - 1, 3)])
    elif name == "two_cliques":                       # two cliques joined by one edge, plus isolated nodes (one of them looped)
        n = 130
        r, c = np.nonzero(np.ones((60, 60)) - np.eye(60))
        twin = _sym_unit(n, np.concatenate([r, r + 60, [0]]), np.concatenate([c, c + 60, [60]]))
        nodes = np.concatenate([[0, 60, 125, n - 1], np.arange(7, 120, 4)])
    else:                                             # complete graph with every loop: no candidate at all
        n = 200
        r, c = np.nonzero(np.ones((n, n)) - np.eye(n))
        twin = _sym_unit(n, r, c)
        nodes = np.arange(n)
    nodes = np.unique(nodes)
    return LoopGraph(name, with_loops(twin, nodes), twin, False, None, None, None)


def _wide_loops():
    """WIDE_NODES nodes, unit and sparse (mean degree about 4): an id space the two-pass scan takes in more than one id window;
    loops on a third of the nodes, the lowest and the highest id among them."""
    rng = np.random.default_rng(23)
    n, m = WIDE_NODES, 2 * WIDE_NODES
    span = rng.integers(1, n, m)                       # (endpoints at every distance: candidates straddle the window boundary)
    r = rng.integers(0, n, m)
    twin = _sym_unit(n, r, (r + span) % n)
    nodes = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < 1 / 3), [0, n - 1]]))
    return LoopGraph("wide_loops", with_loops(twin, nodes), twin, False, None, None, None)


def graph(name):
    """The LoopGraph ``name``: "rmat_loops", "collab_like_loops", "wide_loops" or one of STRUCTURED (cached; do not modify)."""
    if name not in _GRAPHS:
        make = {"rmat_loops": _rmat_loops, "collab_like_loops": _collab_like_loops, "wide_loops": _wide_loops}
        _GRAPHS[name] = make[name]() if name in make else _structured(name)
    return _GRAPHS[name]


def arrays(A, weighted):
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), (A.data.astype(np.float32) if weighted else None)


def node_weights(oracle, A, weighted, kind):
    """float32 weight table of ``kind`` ("aa", "ra", "cn") from the oracle's column sums (the loop counts in them)."""
    rp, col, val = arrays(A, weighted)
    n = A.shape[0]
    if kind == "cn":
        return np.ones(n, np.float32)
    return oracle.node_weights(oracle.col_sums(rp, col, val, n), {"aa": oracle.W_AA, "ra": oracle.W_RA}[kind])


def score_pairs(oracle, A, weighted, kind, pairs, weights=None):
    """Truth of the listed pairs [E, 2] under ``weights`` (default: the graph's own table of ``kind``)."""
    rp, col, val = arrays(A, weighted)
    w = node_weights(oracle, A, weighted, kind) if weights is None else weights
    count, cn, f32 = oracle.pair_scores(rp, col, val, w, pairs[:, 0], pairs[:, 1])
    _, f64 = oracle.pair_scores_f64(rp, col, val, w.astype(np.float64), pairs[:, 0], pairs[:, 1])
    return Truth(pairs, count, cn, f32, f64, w)


def truth(oracle, name, kind, twin=False):
    """Truth of every candidate of a graph (or of its twin), column-major: the pairs, the number of common neighbours, the
    reference's CN value, the oracle's float32 score and the float64-accumulated one, the weight table (cached)."""
    key = (name, kind, twin)
    if key not in _TRUTHS:
        lg = graph(name)
        A = lg.twin if twin else lg.A
        base = (name, "pairs", twin)
        if base not in _TRUTHS:
            _TRUTHS[base] = oracle.candidates_scipy(A)
        pairs, paths = _TRUTHS[base]
        t = score_pairs(oracle, A, lg.weighted, kind, pairs)
        if not lg.weighted:
            assert np.array_equal(t.count, paths.astype(np.int64)), "A @ A and the oracle's pair counts disagree"
        _TRUTHS[key] = t
    return _TRUTHS[key]


def first_rows(t, k, scores=None):
    """Indices of the first ``k`` rows of the declared order (score descending, ties in candidate order) over a Truth."""
    s = t.f64 if scores is None else scores
    return np.argsort(-np.asarray(s, np.float64), kind="stable")[:k]


def hubs_first_order(A):
    """Nodes by falling degree, ties by id (the diagonal entry counts in the degree): CSRGraph.degree_ordered's order."""
    return np.argsort(-np.diff(A.indptr), kind="stable")
