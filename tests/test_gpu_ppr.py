"""GPU: personalized PageRank by the fixed-point push (csrc/ppr_push.hip) -- every output of eps_ppr_push against the numpy truth
(tests/ppr_truth.py) bit for bit on both table paths, the LDS overflow redo, rows on both sides of the whole-workgroup walk, the
saturated threshold, the edge cases, determinism under reordering and splits, the pair and the column entry and the bound between
them, and filter.py / rank.py --model ppr end to end on the scaled stand-ins.  On the parent of this change none of the names
exist."""
import argparse

import numpy as np
import pytest
import torch

import ppr_truth as pt
from test_gpu_katz_filter import CASES, _graph, _stand_in

pytestmark = pytest.mark.gpu

MAX_ROUNDS = 1024
_MEMO = {}


def _truth(key, rowptr, col, s, a16, thr, max_rounds=MAX_ROUNDS):
    """pt.push of one source, computed once per (graph key, source, parameters) and left unchanged."""
    k = (key, int(s), a16, thr, max_rounds)
    if k not in _MEMO:
        bk = (key, "bars", thr)
        if bk not in _MEMO:
            _MEMO[bk] = pt.thresholds(np.diff(rowptr), thr)
        _MEMO[k] = pt.push(rowptr, col, int(s), a16, thr, max_rounds, _MEMO[bk])
    return _MEMO[k]


def _truth_queries(key, rowptr, col, sources, qptr, qnode, a16, thr, max_rounds=MAX_ROUNDS):
    mass = np.zeros(len(qnode), np.int64)
    per = np.zeros((4, len(sources)), np.int64)
    for i, s in enumerate(np.asarray(sources).tolist()):
        p, _, per[0, i], per[1, i], per[2, i], per[3, i] = _truth(key, rowptr, col, s, a16, thr, max_rounds)
        mass[qptr[i]:qptr[i + 1]] = p[qnode[qptr[i]:qptr[i + 1]]]
    return mass, per[0].astype(np.int32), per[1], per[2], per[3].astype(np.int32)


def _push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, max_rounds=MAX_ROUNDS, table="auto", stats=None):
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(dev)
    out = eps.ops.ppr_push(t(rowptr, torch.int64), t(col, torch.int32), len(rowptr) - 1, t(sources, torch.int32), t(qptr, torch.int64),
                           t(qnode, torch.int32), a16, thr, max_rounds, table=table, stats=stats)
    assert [o.dtype for o in out] == [torch.int64, torch.int32, torch.int64, torch.int64, torch.int32]
    return tuple(o.cpu().numpy() for o in out)


def _assert_bitwise(got, want, what):
    for name, g, w in zip(("mass", "rounds", "pushes", "steps", "capped"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(g != w)[:8]}"


def _all_queries(n, n_sources):
    return np.arange(n_sources + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int32), n_sources)


def _star(leaves, tail=0):
    """Node 0 joined to nodes 1 .. leaves, then a path of ``tail`` further nodes (a component of its own); symmetric."""
    n = 1 + leaves + tail
    src = [np.zeros(leaves, np.int64), np.arange(1, leaves + 1)]
    dst = [np.arange(1, leaves + 1), np.zeros(leaves, np.int64)]
    if tail > 1:
        a = np.arange(1 + leaves, n - 1)
        src += [a, a + 1]; dst += [a + 1, a]
    return _csr(n, np.concatenate(src), np.concatenate(dst))


def _csr(n, src, dst):
    order = np.lexsort((dst, src))
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=rowptr[1:])
    return rowptr, dst[order].astype(np.int32)


# ------------------------------------------------------------------------------------------------- bitwise against the truth
@pytest.mark.parametrize("name", pt.SYMMETRIC_GOLDEN)
def test_every_node_a_source_and_a_query(eps, dev, name):
    """eps' = 2^-10, alpha = 0.15: all five outputs, on both table paths."""
    rowptr, col, val = pt.golden_graph(name)
    assert (name == "collab_like") == bool(np.any(val != 1.0))              # (values present there, and ignored)
    n = len(rowptr) - 1
    a16, thr = 9830, 1 << 38
    sources = np.arange(n, dtype=np.int32)
    qptr, qnode = _all_queries(n, n)
    want = _truth_queries(name, rowptr, col, sources, qptr, qnode, a16, thr)
    assert want[1].max() >= 1
    for table in ("auto", "global"):
        _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, table=table), want, f"{name} {table}")


@pytest.mark.parametrize("alpha", [0.15, 0.5])
@pytest.mark.parametrize("e", [1e-4, 1e-6])
@pytest.mark.parametrize("name", pt.SYMMETRIC_GOLDEN)
def test_seeded_sources(eps, dev, name, e, alpha):
    """64 seeded sources (repeats on the small graphs), every node a query."""
    rowptr, col, _ = pt.golden_graph(name)
    n = len(rowptr) - 1
    a16, thr = pt.parameters(alpha, e)
    sources = np.random.default_rng(11).integers(0, n, 64).astype(np.int32)
    qptr, qnode = _all_queries(n, 64)
    want = _truth_queries(name, rowptr, col, sources, qptr, qnode, a16, thr)
    assert want[4].max() == 0
    for table in ("auto", "global"):
        _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, table=table), want, f"{name} {e} {alpha} {table}")


# ------------------------------------------------------------------------------------------------- table paths
def test_lds_overflow_is_redone_in_the_global_table(eps, dev):
    """A star with lds_nodes + 1000 leaves sourced at the hub (its row alone is beyond the LDS table) and at a leaf (the table
    fills in round 2 and the source is redone from the start), in one call with small sources that stay in LDS."""
    lds_nodes = eps.ops.ppr_push_limits(0)[0]
    leaves = lds_nodes + 1000
    rowptr, col = _star(leaves, tail=40)
    n = len(rowptr) - 1
    a16, thr = pt.parameters(0.15, 1e-4)
    small = [n - 1, n - 7, n - 20, n - 33]
    sources = np.array([small[0], 0, small[1], 17, small[2], leaves, small[3]], np.int32)
    qptr, qnode = _all_queries(n, len(sources))
    want = _truth_queries("star_overflow", rowptr, col, sources, qptr, qnode, a16, thr)
    st = {}
    got = _push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, stats=st)
    _assert_bitwise(got, want, "overflow redo")
    assert st["global_sources"] == 3                                        # the hub and the two leaves; the path's nodes stayed in LDS
    touched = [(np.asarray(_truth("star_overflow", rowptr, col, s, a16, thr)[0]) > 0).sum() for s in (0, 17, n - 1)]
    assert touched[0] > lds_nodes and touched[1] > lds_nodes and touched[2] < 64
    _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, table="global"), want, "overflow, forced global")


def test_rows_on_both_sides_of_the_whole_workgroup_walk(eps, dev):
    """Two joined hubs with big_row and big_row + 1 entries (the last row a wave flattens, the first the workgroup walks
    together: longer than anything the kernel stages), sourced at the hubs and at a leaf of each."""
    big = eps.ops.ppr_push_limits(0)[1]
    a_leaves, b_leaves = big - 1, big                                        # hub A = 0: leaves + B; hub B = 1: leaves + A
    n = 2 + a_leaves + b_leaves
    la, lb = np.arange(2, 2 + a_leaves), np.arange(2 + a_leaves, n)
    src = np.concatenate([[0, 1], np.zeros(a_leaves, np.int64), la, np.ones(b_leaves, np.int64), lb])
    dst = np.concatenate([[1, 0], la, np.zeros(a_leaves, np.int64), lb, np.ones(b_leaves, np.int64)])
    rowptr, col = _csr(n, src, dst)
    assert rowptr[1] - rowptr[0] == big and rowptr[2] - rowptr[1] == big + 1
    a16, thr = pt.parameters(0.15, 1e-8)
    sources = np.array([0, 1, 2, n - 1], np.int32)
    qnode = np.concatenate([np.arange(0, 40), np.arange(n - 40, n)]).astype(np.int32)
    qptr = np.arange(5, dtype=np.int64) * len(qnode)
    qnode = np.tile(qnode, 4)
    want = _truth_queries("two_hubs", rowptr, col, sources, qptr, qnode, a16, thr)
    assert want[4].max() == 0 and want[3].min() > 2 * big                   # both hubs pushed, for every source
    _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr), want, "two hubs")


def test_saturated_threshold(eps, dev):
    """T d(hub) = 2^47 (2^17 + 1) passes 2^63 and, taken modulo 2^64, comes back to 2^47: the hub must never push."""
    leaves = (1 << 17) + 1
    rowptr, col = _star(leaves)
    n = len(rowptr) - 1
    a16, thr = pt.parameters(0.15, 0.5)
    assert thr == 1 << 47 and thr * leaves > 1 << 63 and (thr * leaves) % (1 << 64) == 1 << 47
    sources = np.array([5, 0], np.int32)
    qnode = np.array([0, 5, 6, 0, 5], np.int32)
    qptr = np.array([0, 3, 5], np.int64)
    want = _truth_queries("star_saturated", rowptr, col, sources, qptr, qnode, a16, thr)
    assert want[1].tolist() == [1, 0] and want[0].tolist() == [0, int(pt.ONE * 9830) >> 16, 0, 0, 0]
    for table in ("auto", "global"):
        _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, table=table), want, f"saturated {table}")


# ------------------------------------------------------------------------------------------------- edges
def test_edge_cases(eps, dev):
    rowptr, col, _ = pt.golden_graph("isolated_deg1")
    deg = np.diff(rowptr)
    n = len(rowptr) - 1
    a16, thr = pt.parameters(0.15, 1e-4)
    iso = int(np.flatnonzero(deg == 0)[0])
    live = int(np.flatnonzero(deg > 0)[0])
    far = [x for x in range(n) if _truth("isolated_deg1", rowptr, col, live, a16, thr)[0][x] == 0 and x != iso][0]
    # an empty query list; an isolated source asked for itself and another node; a node never touched; duplicate queries;
    # duplicate sources
    sources = np.array([live, iso, live, live], np.int32)
    qptr = np.array([0, 0, 2, 5, 8], np.int64)
    qnode = np.array([iso, live, far, live, far, live, live, int(col[rowptr[live]])], np.int32)
    want = _truth_queries("isolated_deg1", rowptr, col, sources, qptr, qnode, a16, thr)
    assert want[0][0] == pt.ONE and want[0][1] == 0 and want[0][2] == 0 and want[0][3] > 0 and want[0][5] == want[0][6]
    for table in ("auto", "global"):
        _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, table=table), want, f"edges {table}")
    # zero sources
    got = _push(eps, dev, rowptr, col, np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), a16, thr)
    assert [len(g) for g in got] == [0, 0, 0, 0, 0]
    t = lambda x, dt: torch.as_tensor(x, dtype=dt).to(dev)
    with pytest.raises(eps.EpsError, match="sources must lie"):
        eps.ops.ppr_push(t(rowptr, torch.int64), t(col, torch.int32), n, t([n], torch.int32), t([0, 0], torch.int64),
                         torch.zeros(0, dtype=torch.int32, device=dev), a16, thr, 8)
    with pytest.raises(eps.EpsError, match="query nodes must lie"):
        eps.ops.ppr_push(t(rowptr, torch.int64), t(col, torch.int32), n, t([0], torch.int32), t([0, 1], torch.int64),
                         t([-1], torch.int32), a16, thr, 8)


def test_max_rounds_caps_and_says_so(eps, dev):
    rowptr, col, _ = pt.golden_graph("path30")
    n = len(rowptr) - 1
    a16, thr = pt.parameters(0.15, 1e-4)
    sources = np.array([0, 15, 29], np.int32)
    qptr, qnode = _all_queries(n, 3)
    want = _truth_queries("path30", rowptr, col, sources, qptr, qnode, a16, thr, max_rounds=3)
    assert want[1].tolist() == [3, 3, 3] and want[4].tolist() == [1, 1, 1]
    for table in ("auto", "global"):
        _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, max_rounds=3, table=table), want, f"capped {table}")
    one = _truth_queries("path30", rowptr, col, sources, qptr, qnode, a16, thr, max_rounds=1)
    _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr, max_rounds=1), one, "one round")


# ------------------------------------------------------------------------------------------------- determinism and splits
def test_launches_orders_and_splits_give_the_same_bits(eps, dev):
    rowptr, col, _ = pt.golden_graph("rmat10")
    n = len(rowptr) - 1
    a16, thr = pt.parameters(0.15, 1e-5)
    rng = np.random.default_rng(3)
    sources = rng.integers(0, n, 200).astype(np.int32)
    counts = rng.integers(0, 40, 200)
    qptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    qnode = rng.integers(0, n, int(qptr[-1])).astype(np.int32)
    first = _push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr)
    _assert_bitwise(_push(eps, dev, rowptr, col, sources, qptr, qnode, a16, thr), first, "second launch")
    # reversed
    rq = [qnode[qptr[i]:qptr[i + 1]] for i in range(199, -1, -1)]
    rptr = np.r_[0, np.cumsum(counts[::-1])].astype(np.int64)
    rev = _push(eps, dev, rowptr, col, sources[::-1], rptr, np.concatenate(rq), a16, thr)
    for k in range(1, 5):
        assert np.array_equal(rev[k][::-1], first[k])
    for i in range(200):
        assert np.array_equal(rev[0][rptr[199 - i]:rptr[200 - i]], first[0][qptr[i]:qptr[i + 1]])
    # split in two calls
    a = _push(eps, dev, rowptr, col, sources[:77], qptr[:78], qnode[:qptr[77]], a16, thr)
    b = _push(eps, dev, rowptr, col, sources[77:], qptr[77:] - qptr[77], qnode[qptr[77]:], a16, thr, table="global")
    _assert_bitwise(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), first, "split")


# ------------------------------------------------------------------------------------------------- pair entry
def _dev_graph(eps, dev, name):
    from eps_amd.graph import CSRGraph
    rowptr, col, val = pt.golden_graph(name)
    n = len(rowptr) - 1
    return CSRGraph(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev), n, n), rowptr, col


def _pair_truth(key, rowptr, col, u, v, a16, thr):
    m_uv = np.array([_truth(key, rowptr, col, a, a16, thr)[0][b] for a, b in zip(u.tolist(), v.tolist())], np.int64)
    m_vu = np.array([_truth(key, rowptr, col, b, a16, thr)[0][a] for a, b in zip(u.tolist(), v.tolist())], np.int64)
    return pt.pair_score(m_uv, m_vu)


@pytest.mark.parametrize("name", ["er500", "collab_like"])
def test_pair_entry_is_the_truths_formula_and_symmetric(eps, dev, name):
    from eps_amd import heuristics, models
    g, rowptr, col = _dev_graph(eps, dev, name)
    n = g.n_rows
    a16, thr = pt.parameters(0.15, 1e-4)
    rng = np.random.default_rng(5)
    u, v = rng.integers(0, n, 700), rng.integers(0, n, 700)
    u[600:], v[600:] = u[:100], v[:100]                                      # repeats
    u[590:600] = v[590:600]                                                  # self pairs
    e = torch.from_numpy(np.stack([u, v]))
    st = {}
    got = heuristics.ppr(g, e, device_out=True, stats=st)
    assert got.dtype == torch.float32 and got.is_cuda and st["capped"] == 0 and st["sources"] == len(set(u.tolist()) | set(v.tolist()))
    want = _pair_truth(name, rowptr, col, u, v, a16, thr)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)) and want.max() > 0
    back = heuristics.ppr(g, e.flip(0), device_out=True)
    assert torch.equal(back.view(torch.int32), got.view(torch.int32))
    assert torch.equal(heuristics.ppr(g, e).view(torch.int32), got.cpu().view(torch.int32))      # (host output by default)
    other = heuristics.ppr(g, e, alpha=0.5, eps=1e-6, device_out=True)
    assert np.array_equal(other.cpu().numpy().view(np.int32), _pair_truth(name, rowptr, col, u, v, *pt.parameters(0.5, 1e-6)).view(np.int32))
    # the module's forward returns it: no sigmoid, no parameters
    m = models.CommonNeighborsPredictor(None, 0, 0, 0, 1, 0.0, model_type="ppr").to(dev)
    assert torch.equal(m(None, e.to(dev), g).view(torch.int32), got.view(torch.int32))


# ------------------------------------------------------------------------------------------------- column entry and routes
def _two_hop_lists(rowptr, col):
    """(colptr, cand_u): for every column v its 2-hop non-edges u != v, ascending."""
    import scipy.sparse as sp
    n = len(rowptr) - 1
    A = sp.csr_matrix((np.ones(len(col)), col, rowptr), shape=(n, n))
    two = ((A @ A) > 0).astype(np.int8) - ((A @ A) > 0).multiply(A > 0).astype(np.int8)
    two.setdiag(0); two.eliminate_zeros()
    two = two.T.tocsr(); two.sort_indices()
    return two.indptr.astype(np.int64), two.indices.astype(np.int32)


@pytest.mark.parametrize("name", ["er500", "rmat10"])
def test_column_entry_is_its_formula_and_within_the_bound_of_the_pair_entry(eps, dev, name):
    from eps_amd import heuristics
    g, rowptr, col = _dev_graph(eps, dev, name)
    n = g.n_rows
    deg = np.diff(rowptr)
    a16, thr = pt.parameters(0.15, 1e-4)
    colptr, cand_u = _two_hop_lists(rowptr, col)
    v_of = np.repeat(np.arange(n), np.diff(colptr))
    assert len(cand_u) > 10 * n
    got = heuristics.ppr_columns(g, 0, n, colptr, cand_u, device_out=True)
    m_vu = np.concatenate([_truth(name, rowptr, col, v, a16, thr)[0][cand_u[colptr[v]:colptr[v + 1]]] for v in range(n)])
    want = pt.column_score(m_vu, deg[cand_u], deg[v_of])
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    # a block of columns in the middle, as a filter hands it over: the same bits
    lo, hi = n // 3, n // 3 + 97
    part = heuristics.ppr_columns(g, lo, hi, colptr[lo:hi + 1] - colptr[lo], cand_u[colptr[lo]:colptr[hi]], device_out=True)
    assert np.array_equal(part.cpu().numpy().view(np.int32), want[colptr[lo]:colptr[hi]].view(np.int32))
    # the two routes: |column - pair| < eps' d(v) plus one float32 ulp of the larger
    pair = heuristics.ppr(g, torch.from_numpy(np.stack([cand_u.astype(np.int64), v_of]))).numpy()
    c = got.cpu().numpy()
    big = np.maximum(np.abs(c), np.abs(pair))
    ulp = np.nextafter(big, np.float32(np.inf)) - big
    gap = np.abs(c.astype(np.float64) - pair.astype(np.float64))
    assert np.all(gap < thr * 2.0 ** -48 * deg[v_of] + ulp), float((gap / (thr * 2.0 ** -48 * deg[v_of])).max())
    assert gap.max() > 0                                                    # (not bitwise the same score, and not claimed to be)


def test_column_entry_refuses_an_asymmetric_pattern(eps, dev):
    from eps_amd import heuristics
    from eps_amd.graph import CSRGraph
    rowptr, col = _csr(4, np.array([0, 1, 2, 2]), np.array([1, 2, 0, 3]))
    g = CSRGraph(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), None, 4, 4)
    with pytest.raises(eps.EpsError, match="symmetric"):
        heuristics.ppr_columns(g, 0, 4, np.array([0, 1, 1, 1, 1]), np.array([2], np.int32))
    # the pair entry takes it: a node without entries (3) never pushes, so what it receives stays residual
    a16, thr = pt.parameters(0.15, 1e-4)
    got = heuristics.ppr(g, torch.tensor([[0, 2, 3], [2, 3, 0]])).numpy()
    want = _pair_truth("directed4", rowptr, col, np.array([0, 2, 3]), np.array([2, 3, 0]), a16, thr)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and got[0] > 0 and got[1] == 0 and got[2] == 0


# ------------------------------------------------------------------------------------------------- CLI
_RUNS = {}


def _filter(dataset, run, *flags):
    from eps_amd import filter_stage
    return torch.load(filter_stage.main(["--dataset", dataset, "--model", "ppr", "--checkpoint", f"{dataset}_ppr||0|{run}.pt",
                                         "--synthetic", *flags]))


EPS_FLAGS = {"default": (), "1e-6": ("--ppr_eps", "1e-6")}


def _full(tmp_path_factory, which="1e-6"):
    """(work directory, the full file) of the bare command, or of --ppr_eps 1e-6: one run each, shared by the tests below.  The ddi
    stand-in is dense (mean degree near 300): at the default eps = 1e-4 no neighbour of a source reaches its own threshold
    ((1 - alpha) / d < eps d), every candidate's mass is 0 and so is every score -- the truth says the same; at 1e-6 the scores
    order the candidates."""
    if which not in _RUNS:
        workdir = tmp_path_factory.mktemp(f"ppr_ddi_{len(_RUNS)}")
        with _stand_in("ddi", workdir):
            _RUNS[which] = (workdir, _filter("ddi", 0, *EPS_FLAGS[which]))
    return _RUNS[which]


@pytest.mark.parametrize("which", sorted(EPS_FLAGS))
def test_filter_full_file(eps, dev, oracle, tmp_path_factory, which):
    """filter.py --dataset ddi --model ppr --synthetic [--ppr_eps 1e-6]: the 2-hop non-edge set, every score the column entry's
    truth bit for bit, rows in the declared order."""
    from oracle import eps_oracle
    workdir, rows = _full(tmp_path_factory, which)
    with _stand_in("ddi", workdir):
        A = _graph(oracle, "ddi").tocsr()
    A.sort_indices()
    n = A.shape[0]
    rowptr, col = A.indptr.astype(np.int64), A.indices.astype(np.int32)
    rows = rows.numpy()
    assert rows.dtype == np.float32 and rows.shape == (CASES["ddi"][2], 3) and n == CASES["ddi"][1]
    u, v, s = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2]
    cand = eps_oracle.candidates_scipy(A)[0]
    assert np.array_equal(np.sort(v * n + u), np.sort(cand[:, 1] * n + cand[:, 0]))
    a16, thr = pt.parameters(0.15, 1e-4 if which == "default" else 1e-6)
    deg = np.diff(rowptr)
    P = np.stack([_truth("ddi_stand_in", rowptr, col, x, a16, thr)[0] for x in range(n)])
    want = pt.column_score(P[v, u], deg[u], deg[v])
    assert np.array_equal(s.view(np.int32), want.view(np.int32))
    assert np.array_equal(np.lexsort((u, v, -s.astype(np.float64))), np.arange(len(s)))
    if which == "1e-6":
        assert s.min() > 0 and len(np.unique(s)) > len(s) // 4


def test_filter_keep_top_and_keep_per_node_are_cuts_of_the_full_file(eps, dev, tmp_path_factory):
    workdir, rows = _full(tmp_path_factory)
    with _stand_in("ddi", workdir):
        top = _filter("ddi", 1, "--keep_top", "1000", *EPS_FLAGS["1e-6"])
        cut = _filter("ddi", 2, "--keep_per_node", "3", *EPS_FLAGS["1e-6"])
    assert top.shape == (1000, 3) and torch.equal(top, rows[:1000])
    v = rows[:, 1].numpy().astype(np.int64)
    order = np.argsort(v, kind="stable")
    start = np.r_[0, np.flatnonzero(np.diff(v[order])) + 1]
    rank = np.arange(len(v)) - np.repeat(start, np.diff(np.r_[start, len(v)]))
    keep = np.zeros(len(v), bool)
    keep[order[rank < 3]] = True
    assert 0 < keep.sum() < len(v) and torch.equal(cut, rows[torch.from_numpy(keep)])


def test_two_ranks_write_the_single_process_file(eps, dev, tmp_path_factory):
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _rank_main
    workdir, rows = _full(tmp_path_factory)
    with _stand_in("ddi", workdir):
        argv = ["--dataset", "ddi", "--model", "ppr", "--checkpoint", "ddi_ppr||0|4.pt", "--synthetic", *EPS_FLAGS["1e-6"]]
        mp.spawn(_rank_main, args=(2, _free_port(), str(workdir), argv), nprocs=2, join=True)
        multi = torch.load("filtered_edges/ddi_ppr__0_4_sorted_edges.pt")
    assert torch.equal(multi, rows)


def test_rank_cli_and_the_hits_table_of_the_truth(eps, dev, tmp_path, monkeypatch):
    """rank.py --dataset collab --model ppr --synthetic --runs 1: finite Hits in [0, 100]; and on a sub-sampled split (200 rows
    per list) evaluate.test gives exactly the table the truth's scores give."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", CASES["collab"][0])
    from eps_amd import datasets, evaluate, models, rank_stage
    from eps_amd.graph import add_edges
    from eps_amd.rank_helpers import to_undirected
    curves = rank_stage.main(["--dataset", "collab", "--model", "ppr", "--synthetic", "--runs", "1"])
    assert len(curves) == 1 and int(curves[0][0]) == 0
    for x in curves[0][1:]:
        assert np.isfinite(float(x)) and 0.0 <= float(x) <= 100.0
    args = models.default_model_configs(argparse.Namespace(
        dataset="collab", model="ppr", synthetic=True, num_layers=None, hidden_channels=None, dropout=None, batch_size=None,
        lr=None, epochs=None, use_feature=None, use_learnable_embedding=None))
    edge_index, edge_weight, split_edge, data = datasets.get_data(args)
    data = data.to(dev)
    ei, ew = edge_index.to(dev), edge_weight.to(dev)
    data.adj_t = add_edges("collab", ei, ew, ei.new_zeros((2, 0)), data.num_nodes)
    data.full_adj_t = add_edges("collab", ei, ew, to_undirected(split_edge['valid']['edge'].t()).to(dev), data.num_nodes)
    assert data.adj_t.val is not None and bool((data.adj_t.val != 1).any())  # (stored values present, and ignored)
    sub = {"eval_train": {"edge": split_edge["eval_train"]["edge"][:200]},
           "valid": {"edge": split_edge["valid"]["edge"][:200], "edge_neg": split_edge["valid"]["edge_neg"][:200]},
           "test": {"edge": split_edge["test"]["edge"][:200], "edge_neg": split_edge["test"]["edge_neg"][:200]}}
    model = models.build_model(args, data, dev)
    got = evaluate.test(model, data, sub, evaluate.evaluators["collab"], 1 << 16, args, dev)
    a16, thr = pt.parameters(0.15, 1e-4)

    def scores(key, g, edges):
        rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
        e = edges.numpy()
        return torch.from_numpy(_pair_truth(key, rowptr, col, e[:, 0], e[:, 1], a16, thr))

    want = evaluate._hits_table("collab", evaluate.evaluators["collab"], scores("collab_adj", data.adj_t, sub["eval_train"]["edge"]),
                                scores("collab_adj", data.adj_t, sub["valid"]["edge"]), scores("collab_adj", data.adj_t, sub["valid"]["edge_neg"]),
                                scores("collab_full", data.full_adj_t, sub["test"]["edge"]),
                                scores("collab_full", data.full_adj_t, sub["test"]["edge_neg"]))
    assert got == want and set(got) == {"Hits@10", "Hits@50", "Hits@100"}
    for triple in got.values():
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in triple)
