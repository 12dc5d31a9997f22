"""GPU: the sketch kernels (csrc/sketch.hip) against tests/sketch_truth.py, bit for bit -- own sketches, the propagated tables on
a graph built around the kernel's row chunk, and the packed pair statistics on the graph's tables and on synthetic tables that
reach the bounds of the packed fields."""
import numpy as np
import pytest
import torch

import sketch_truth as st

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().view(torch.int32).numpy().view(np.uint32) if t.dtype == torch.uint32 else t.cpu().numpy()


def _dev_tables(hll, mh, dev):
    return (torch.from_numpy(np.ascontiguousarray(hll)).to(dev),
            torch.from_numpy(np.ascontiguousarray(mh).view(np.int32)).view(torch.uint32).to(dev))


@pytest.fixture(scope="module")
def boundary(eps, dev):
    """The boundary graph of the kernel's own row chunk, its truth tables (computed once), and the graph on the device."""
    from eps_amd import ops
    rc, ppw = ops.sketch_limits()
    A, classes = st.boundary_graph(rc)
    hll, mh = st.tables(A, 2)
    g = eps.CSRGraph(torch.from_numpy(A.indptr.astype(np.int64)).to(dev), torch.from_numpy(A.indices.astype(np.int32)).to(dev), None,
                     A.shape[0], A.shape[1])
    return dict(rc=rc, ppw=ppw, A=A, classes=classes, hll=hll, mh=mh, g=g)


# ---------------------------------------------------------------------------------------------------------- own sketches
@pytest.mark.parametrize("first,n", [(0, 1000), (6598086 - 65, 130), ((1 << 31) - 130, 130)])
def test_own_sketches_equal_the_truth(eps, dev, first, n):
    from eps_amd import ops
    hll, mh = ops.sketch_own(first, n, dev)
    want_h, want_m = st.own_sketch(np.arange(first, first + n, dtype=np.uint64))
    assert hll.shape == (n, 256) and mh.shape == (n, 128)
    assert np.array_equal(_np(hll), want_h) and np.array_equal(_np(mh), want_m)
    if first <= 6598086 < first + n:
        assert int(hll[6598086 - first].max()) == 29
    with pytest.raises(eps.EpsError):
        ops.sketch_own((1 << 31) - 1, 2, dev)
    assert ops.sketch_own(5, 0, dev)[0].shape == (0, 256)


# ---------------------------------------------------------------------------------------------------------- propagate
def test_propagated_tables_equal_the_truth(eps, dev, boundary):
    from eps_amd import ops
    A, rc, g = boundary["A"], boundary["rc"], boundary["g"]
    n = A.shape[0]
    # (host side, before any launch) the graph holds every length class and the layouts the piecewise path distinguishes
    deg = np.diff(A.indptr)
    for c, k in st.boundary_lengths(rc).items():
        assert (deg == k).any() and boundary["classes"][c], c
    assert n < 2000 and n % 4 and n % 64 and A[0, 0] != 0
    assert A.indptr[n - 1] == A.indptr[n] and (A.indices == n - 1).any()           # only ever a neighbour
    assert A.indptr[1] % rc == 0 and deg[1] > rc                                     # a long row that begins on a cut
    assert int(A.indices.max()) < n and int(A.indices.min()) >= 0
    b, e = A.indptr[st.LONGEST_ROW], A.indptr[st.LONGEST_ROW + 1]
    assert (e - 1) // rc - b // rc == 4                                              # five pieces: the combine loop's second trip
    own = ops.sketch_own(0, n, dev)
    h1 = ops.sketch_propagate(g.rowptr, g.col, n, own[0], own[1], keep_own=False)
    h2 = ops.sketch_propagate(g.rowptr, g.col, n, h1[0], h1[1], keep_own=True)
    for k, got in enumerate((h1, h2)):
        bad = np.flatnonzero((_np(got[0]) != boundary["hll"][k]).any(1) | (_np(got[1]) != boundary["mh"][k]).any(1))
        assert bad.size == 0, f"hop {k + 1}: rows {bad[:10]} (degrees {deg[bad[:10]]}) differ from the truth"
    # the same bits on a second run, and through CSRGraph.sketches (one [K, n, .] table, written in place)
    again = ops.sketch_propagate(g.rowptr, g.col, n, own[0], own[1], keep_own=False)
    assert torch.equal(again[0], h1[0]) and torch.equal(again[1].view(torch.int32), h1[1].view(torch.int32))
    hll, mh, card = g.sketches(2)
    assert np.array_equal(_np(hll), boundary["hll"]) and np.array_equal(_np(mh), boundary["mh"])
    assert g.sketches(2)[0] is hll and g.sketches(1)[0].shape == (1, n, 256)
    assert np.array_equal(_np(g.sketches(1)[1]), boundary["mh"][:1])
    want = st.row_cardinality(boundary["hll"])
    assert card.dtype == torch.float64 and card.shape == (2, n)
    assert np.allclose(card.cpu().numpy(), want, rtol=1e-14, atol=0) and float(card[0, 3]) == 0.0
    # refusals: aliased output, an entry outside the graph
    with pytest.raises(eps.EpsError, match="alias"):
        ops.sketch_propagate(g.rowptr, g.col, n, own[0], own[1], keep_own=False, out=own)
    bad_col = g.col.clone()
    bad_col[7] = n
    with pytest.raises(eps.EpsError, match="col"):
        ops.sketch_propagate(g.rowptr, bad_col, n, own[0], own[1], keep_own=False)


# ---------------------------------------------------------------------------------------------------------- pair statistics
def _check_stats(ops, tabs, truth, n, u, v, dev):
    ut, vt = torch.from_numpy(u.astype(np.int32)).to(dev), torch.from_numpy(v.astype(np.int32)).to(dev)
    S, Z, M = ops.sketch_pair_stats(tabs[0], tabs[1], n, ut, vt, check=False)
    wS, wZ, wM = st.pair_stats(truth[0], truth[1], u, v)
    K = truth[0].shape[0]
    assert S.shape == Z.shape == M.shape == (len(u), K, K) and S.dtype == torch.int64 and Z.dtype == M.dtype == torch.int32
    assert np.array_equal(S.cpu().numpy(), wS) and np.array_equal(Z.cpu().numpy(), wZ) and np.array_equal(M.cpu().numpy(), wM)
    return S, Z, M


@pytest.mark.parametrize("K", [1, 2])
def test_pair_statistics_on_the_graph_tables(eps, dev, boundary, K):
    from eps_amd import ops
    A, cls = boundary["A"], boundary["classes"]
    n = A.shape[0]
    truth = (boundary["hll"][:K], boundary["mh"][:K])
    tabs = _dev_tables(*truth, dev)
    rng = np.random.default_rng(8)
    iso, hubs = cls["0"][0], cls["2rc+1"] + cls["rc+1"]
    assert not (boundary["hll"][1][iso].any())                                     # isolated at both hops
    special_u = np.array([iso, iso, 5, 9, 9, hubs[0], hubs[0], hubs[1], n - 1, 0])
    special_v = np.array([iso, 5, iso, 9, 4, hubs[1], hubs[0], hubs[2], 0, n - 1])
    for B in (0, 1, 3, 4, 5, 63, 64, 65, 1000):
        u = np.concatenate([special_u, rng.integers(0, n, 1000)])[:B]
        v = np.concatenate([special_v, rng.integers(0, n, 1000)])[:B]
        S, Z, M = _check_stats(ops, tabs, truth, n, u, v, dev)
        if B:
            assert (S[0] == 1 << 41).all() and (Z[0] == 256).all() and (M[0] == 128).all()
        # stat(u, v)[i, j] == stat(v, u)[j, i]
        T = _check_stats(ops, tabs, truth, n, v, u, dev)
        assert all(torch.equal(a, b.transpose(1, 2)) for a, b in zip((S, Z, M), T))
    # an id outside the graph: refused under check=True; -1 in its slots and nothing else disturbed under check=False
    u = np.concatenate([special_u, rng.integers(0, n, 90)])
    v = np.concatenate([special_v, rng.integers(0, n, 90)])
    for pos, (bu, bv) in {2: (n, 0), 17: (0, -1), 64: (1 << 30, 3), 99: (-5, n + 7)}.items():
        u[pos], v[pos] = bu, bv
    S, Z, M = _check_stats(ops, tabs, truth, n, u, v, dev)
    bad = np.zeros(len(u), bool)
    bad[[2, 17, 64, 99]] = True
    assert (S[torch.from_numpy(bad).to(dev)] == -1).all() and (S[torch.from_numpy(~bad).to(dev)] >= 0).all()
    with pytest.raises(eps.EpsError, match="node ids"):
        ops.sketch_pair_stats(tabs[0], tabs[1], n, torch.from_numpy(u.astype(np.int32)).to(dev), torch.from_numpy(v.astype(np.int32)).to(dev))


@pytest.mark.parametrize("K", [1, 2])
def test_pair_statistics_on_synthetic_tables_reach_the_field_bounds(eps, dev, K):
    """Random registers in [0, 33] with all-33 and all-0 rows, random words with planted equal words: the only way to the bounds
    of the packed word (S = 2^41 with Z = 256; S = 256 with Z = 0; 0 and 128 matches)."""
    from eps_amd import ops
    rng = np.random.default_rng(21 + K)
    n = 203
    hll = rng.integers(0, 34, (K, n, 256)).astype(np.uint8)
    mh = rng.integers(0, 1 << 32, (K, n, 128), dtype=np.uint64).astype(np.uint32)
    hll[:, 0] = 33
    hll[:, 1] = 0
    hll[:, 2, ::2] = 0
    mh[:, 1] = mh[:, 0]                                                         # 128 matches
    mh[:, 3, :64] = mh[:, 2, :64]                                               # 64 planted
    for r in range(4, 40):                                                      # a few planted words per row pair
        w = rng.choice(128, int(rng.integers(0, 12)), replace=False)
        mh[:, r + 1, w] = mh[:, r, w]
    if K == 2:
        mh[1, 5] = mh[0, 6]
    tabs = _dev_tables(hll, mh, dev)
    u = np.concatenate([[0, 1, 0, 1, 2, 3, 5], np.arange(4, 40), rng.integers(0, n, 400)])
    v = np.concatenate([[0, 1, 1, 0, 3, 2, 6], np.arange(5, 41), rng.integers(0, n, 400)])
    S, Z, M = _check_stats(ops, tabs, (hll, mh), n, u, v, dev)
    assert (S[0] == 256).all() and (Z[0] == 0).all() and (S[1] == 1 << 41).all() and (Z[1] == 256).all()
    assert (M[2].diagonal() == 128).all() and int(M[4, 0, 0]) >= 64 and int(M.min()) == 0
    if K == 2:
        assert int(M[6, 1, 0]) == 128
