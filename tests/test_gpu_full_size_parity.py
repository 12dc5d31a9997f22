"""The headline filter step at full size against independent references: ``scan.scan_topk`` on the ppa-like graph under hubs-first
labels (skipped heads + eps_scan_refine, sketch pieces in the sparse tail) at the benchmark's K = 4 M, compared bit for bit with
the two-pass exact kernel (eps_filter_scan, ``scan.ONE_PASS = False``: no screen, no heads, no sketch) on a SEPARATE graph object,
and column by column with a float64 restatement of filter.py:96-142 (A diag(w) A on the host).  A soak of repeated calls on one
graph object, the full-scale ddi common-neighbour filter against a dense float64 A @ A, and the two regressions of the scan's
status word and of the refine kernel's sums."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_FULL = 4_000_000
NEAR_CUT_ROWS = 1000           # rows at the end of a result whose columns the float64 reference checks
NEAR_CUT_PATHS = 400_000_000   # ... as many of them (nearest the cut first) as fit into this many two-hop paths of host work
PACKED_COLUMNS = 64            # columns whose pieces in the head table's plan are packed (the kind sketch pieces replace)


def _fresh(g0):
    """A graph object of its own over the same tensors: nothing of another object's cache (relabelled copy, screens, head
    tables, screen_variant) is shared."""
    from eps_amd.graph import CSRGraph
    return CSRGraph(g0.rowptr, g0.col, None, g0.n_rows, g0.n_cols)


@pytest.fixture(scope="module")
def ppa(dev):
    from eps_amd import synth
    return synth.ppa_like(seed=3, device=dev)


@pytest.fixture(scope="module")
def weights(ppa, dev):
    from eps_amd import ops
    from eps_amd.heuristics import node_weight_table
    return {"aa": node_weight_table(ppa, ops.W_AA), "ra": node_weight_table(ppa, ops.W_RA),
            "cn": torch.ones(ppa.n_rows, dtype=torch.float32, device=dev)}


class _TwoPass:
    """Reference rows of (weights, K) from the two-pass exact kernel on one graph object of its own (computed once each)."""

    def __init__(self, g0, weights):
        self.g = _fresh(g0)
        self.weights = weights
        self.rows = {}

    def get(self, kind, k):
        from eps_amd import scan
        if (kind, k) not in self.rows:
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(scan, "ONE_PASS", False)
                p, s = scan.scan_topk(self.g, self.weights[kind], k)
                assert scan.screen_variant(scan.scan_graph(self.g)[0]) is None, "the reference must run eps_filter_scan"
                assert scan.scan_graph(self.g)[1] is None
            assert p.shape == (2, k)
            self.rows[(kind, k)] = (p, s)
        return self.rows[(kind, k)]


@pytest.fixture(scope="module")
def two_pass(ppa, weights):
    return _TwoPass(ppa, weights)


class _ColumnTruth:
    """float64 scores of every candidate of a column set: the column-set form of ``oracle.candidates_scipy_columns`` (2-hop
    non-edges of the column: nonzeros of (A @ A)[:, c] without the diagonal and without A's entries) scored as
    (A diag(w) A)[u, c] in float64, w = the oracle's node weights (common neighbours: 1)."""

    def __init__(self, g, oracle):
        import scipy.sparse as ssp
        A = g.to_scipy()
        self.n = A.shape[0]
        self.rp, self.col = A.indptr.astype(np.int64), A.indices.astype(np.int32)
        self.deg = np.diff(self.rp)
        # (a symmetric pattern: the CSR arrays ARE the CSC arrays of the same matrix)
        self.Ac = ssp.csc_matrix((np.ones(len(self.col)), self.col, self.rp), shape=A.shape)
        self.paths = np.asarray(ssp.csr_matrix((np.ones(len(self.col)), self.col, self.rp), shape=A.shape) @ self.deg.astype(np.float64))
        cs = oracle.col_sums(self.rp, self.col, None, self.n)
        self.w = {"aa": oracle.node_weights(cs, oracle.W_AA), "ra": oracle.node_weights(cs, oracle.W_RA),
                  "cn": np.ones(self.n, np.float32)}
        self.A = A
        self.memo = {}

    def column_set(self, kind, cols):
        """(keys c * n + u ascending, float64 scores) of every candidate (u, c) of the columns ``cols``."""
        import scipy.sparse as ssp
        cols = np.unique(np.asarray(cols, np.int64))
        todo = [c for c in cols.tolist() if (kind, c) not in self.memo]
        w = np.where(self.deg >= 2, self.w[kind].astype(np.float64), 0.0)       # (a common neighbour has two neighbours)
        AD = ssp.csr_matrix((w[self.col], self.col, self.rp), shape=self.A.shape)
        for i in range(0, len(todo), 128):
            chunk = np.array(todo[i:i + 128], np.int64)
            P = (AD @ self.Ac[:, chunk]).tocsc()
            P.eliminate_zeros()
            for j, c in enumerate(chunk.tolist()):
                u = P.indices[P.indptr[j]:P.indptr[j + 1]].astype(np.int64)
                s = P.data[P.indptr[j]:P.indptr[j + 1]]
                known = self.col[self.rp[c]:self.rp[c + 1]]
                keep = (u != c) & ~np.isin(u, known)
                o = np.argsort(u[keep], kind="stable")
                self.memo[(kind, c)] = (c * self.n + u[keep][o], s[keep][o])
        keys = [self.memo[(kind, c)][0] for c in cols.tolist()]
        scs = [self.memo[(kind, c)][1] for c in cols.tolist()]
        return (np.concatenate(keys) if keys else np.zeros(0, np.int64)), (np.concatenate(scs) if scs else np.zeros(0))

    def check(self, kind, pairs, scores, cols, what):
        """The rows of ``pairs`` in the columns ``cols`` are exactly the candidates of those columns above the result's last score
        (ids exact; scores within 1e-5 relative of the float64 truth); candidates within 2e-5 of that score may fall either side."""
        bar = float(scores[-1])
        assert bar > 0.0
        tkey, tsc = self.column_set(kind, cols)
        pu, pv, ps = pairs[0].cpu().numpy(), pairs[1].cpu().numpy(), scores.cpu().numpy()
        m = np.isin(pv, np.asarray(cols, np.int64))
        gkey = pv[m].astype(np.int64) * self.n + pu[m]
        gsc = ps[m]
        assert len(np.unique(gkey)) == len(gkey), f"{what}: a row appears twice"
        sure, maybe = tkey[tsc > bar * (1 + 2e-5)], tkey[tsc > bar * (1 - 2e-5)]
        missing = sure[~np.isin(sure, gkey)]
        assert missing.size == 0, f"{what}: {missing.size} candidates above the cut are missing, e.g. (u, v) = " \
                                  f"{[(int(k % self.n), int(k // self.n)) for k in missing[:5]]}"
        extra = gkey[~np.isin(gkey, maybe)]
        assert extra.size == 0, f"{what}: {extra.size} rows are no candidates above the cut, e.g. " \
                                f"{[(int(k % self.n), int(k // self.n)) for k in extra[:5]]}"
        pos = np.searchsorted(tkey, gkey)
        assert np.array_equal(tkey[pos], gkey)
        want = tsc[pos]
        err = np.abs(gsc.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-30)
        assert float(err.max(initial=0.0)) <= 1e-5, f"{what}: scores differ from the float64 truth by {float(err.max()):.3g}"
        return len(np.unique(np.asarray(cols)))

    def near_cut_columns(self, pairs):
        """The columns of the last NEAR_CUT_ROWS rows (the pairs nearest the cut), nearest first, as many as NEAR_CUT_PATHS of
        host work allow (``near_cut_seen``: how many of how many distinct columns)."""
        pv = pairs[1, -NEAR_CUT_ROWS:].cpu().numpy()[::-1]
        cols, seen, spent = [], set(), 0.0
        for c in pv.tolist():
            if c in seen:
                continue
            seen.add(c)
            if spent + self.paths[c] > NEAR_CUT_PATHS and cols:
                continue
            spent += self.paths[c]
            cols.append(c)
        self.near_cut_seen = (len(cols), len(seen))
        return cols

    def base_columns(self):
        """Hubs, median-degree and tail columns (the dozen test_gpu_scan.py's full-size check looks at)."""
        by_deg = np.argsort(-self.deg, kind="stable")
        n = self.n
        return sorted({int(by_deg[i]) for i in (0, 3, 50, 1000, n // 4, n // 2, n // 2 + 1, 3 * n // 4, n - 1000, n - 2)} | {7, n - 1})


@pytest.fixture(scope="module")
def truth(ppa, oracle):
    return _ColumnTruth(ppa, oracle)


def test_column_truth_is_the_oracle_candidate_set(ppa, oracle, truth):
    """The column-set restatement above against the oracle's own column slice (candidates and float32 pair scores)."""
    lo, hi = 2000, 2040
    cand, _ = oracle.candidates_scipy_columns(truth.A, lo, hi)
    keys, sc = truth.column_set("aa", range(lo, hi))
    want = cand[:, 1] * truth.n + cand[:, 0]
    assert np.array_equal(np.sort(want), keys)
    w = truth.w["aa"]
    _, _, ws = oracle.pair_scores(truth.rp, truth.col, None, w, (keys % truth.n).astype(np.int32), (keys // truth.n).astype(np.int32))
    assert float((np.abs(ws - sc) / np.maximum(sc, 1e-30)).max()) <= 1e-5


def _packed_columns(gs, perm, ht, count, seed):
    """Original ids of ``count`` columns (seeded choice) with at least one packed piece in the head table's plan."""
    pptr, recs = ht.plan
    kind = recs[:, 0] >> 30
    at = torch.nonzero(kind == 1).squeeze(1)
    ptr = pptr.to(torch.int64).bitwise_and(0xFFFFFFFF)
    owner = torch.searchsorted(ptr, at, right=True) - 1
    cols = torch.unique(owner)
    assert cols.numel() >= count, f"only {cols.numel()} columns have packed pieces"
    pick = torch.randperm(cols.numel(), generator=torch.Generator().manual_seed(seed))[:count]
    return sorted(perm[cols.cpu()[pick].to(perm.device)].cpu().tolist())


def test_aa_full_size_step_matches_two_pass_and_float64(ppa, weights, two_pass, truth, dev):
    """Adamic-Adar, K = 4 M, the production path (relabel=True): the graph's first scan (HUB_FIRST hub rows, no column pack) and
    its second (HUB_MAX hub rows, per-column pack) both run skipped heads AND sketch pieces, and both give the two-pass kernel's
    rows and scores bit for bit; the float64 reference agrees on hub / median / tail columns, on columns made of packed pieces and
    on the columns of the rows nearest the cut."""
    from eps_amd import ops, scan
    g = _fresh(ppa)
    w = weights["aa"]
    want_p, want_s = two_pass.get("aa", K_FULL)
    covered = []
    for i in range(2):
        st = {}
        p, s = scan.scan_topk(g, w, K_FULL, relabel=True, stats=st)
        gs, perm = scan.scan_graph(g)
        assert perm is not None
        assert st["heads"], f"scan {i}: skipped heads did not run ({st})"
        assert st["sketch"], f"scan {i}: sketch pieces did not run ({st})"
        assert st["sketch_void"] == 0
        screen = scan.screen_weights(g, gs, perm, w)
        ht = screen.head_cur
        n_hub = scan.hub_rows(gs).shape[0]
        if i == 0:
            assert n_hub <= scan.HUB_FIRST and ht.pack is None
        else:
            assert n_hub == min(ops.HUB_MAX, gs.n_rows) and ht.pack is not None
        assert ht.n_hub == n_hub and ht.wide
        assert torch.equal(p, want_p), f"scan {i}: rows differ from the two-pass kernel's"
        assert torch.equal(s, want_s), f"scan {i}: scores differ from the two-pass kernel's"
        cols = sorted(set(truth.base_columns()) | set(_packed_columns(gs, perm, ht, PACKED_COLUMNS, seed=i))
                      | set(truth.near_cut_columns(p)))
        covered.append((truth.check("aa", p, s, cols, f"AA scan {i}"), truth.near_cut_seen))
    print(f"AA K={K_FULL}: float64 column checks over (columns, (near-cut columns, of)) = {covered}")


@pytest.mark.parametrize("kind", ["ra", "cn"])
@pytest.mark.parametrize("k", [150_000, K_FULL])
def test_ra_cn_full_size_match_two_pass_and_float64(ppa, weights, two_pass, truth, kind, k):
    """Resource allocation and common neighbours on the production path: bit-identical to the two-pass kernel, and the float64
    reference on the base columns and the columns nearest the cut.  Common neighbours screen exactly: no sketch pieces."""
    from eps_amd import scan
    g = _fresh(ppa)
    st = {}
    p, s = scan.scan_topk(g, weights[kind], k, relabel=True, stats=st)
    want_p, want_s = two_pass.get(kind, k)
    assert torch.equal(p, want_p) and torch.equal(s, want_s), f"{kind} K={k}: differs from the two-pass kernel ({st})"
    if kind == "cn":
        assert not st["sketch"], "common neighbours screen exactly: no sketch pieces"
    n = truth.check(kind, p, s, sorted(set(truth.base_columns()) | set(truth.near_cut_columns(p))), f"{kind} K={k}")
    print(f"{kind} K={k}: heads {st['heads']}, sketch {st['sketch']}, float64 column checks over {n} columns "
          f"(near-cut columns {truth.near_cut_seen[0]} of {truth.near_cut_seen[1]})")


def test_soak_one_graph_object_many_bars(ppa, weights, two_pass):
    """30 calls on ONE graph object cycling {AA, RA, CN} x K in a fixed shuffled order: head tables of several bar levels compete
    for the Screen's cache, bar hints and hub tables carry over between calls -- every call equals the two-pass reference of its
    (weights, K).  (A sketch bug that let upper bounds through as CN scores showed up only in a run like this.)"""
    from eps_amd import scan
    g = _fresh(ppa)
    jobs = [(kind, k) for kind in ("aa", "ra", "cn") for k in (1000, 40_000, 150_000, 1_200_000, K_FULL)] * 2
    random.Random(5).shuffle(jobs)
    bad = []
    for i, (kind, k) in enumerate(jobs):
        st = {"count": False}
        p, s = scan.scan_topk(g, weights[kind], k, relabel=True, stats=st)
        want_p, want_s = two_pass.get(kind, k)
        if not (torch.equal(p, want_p) and torch.equal(s, want_s)):
            bad.append((i, kind, k, st.get("heads"), st.get("sketch"), st.get("launches")))
    assert not bad, f"calls that differ from the two-pass reference: {bad}"


def test_ddi_common_neighbours_full_scale_against_dense_float64(eps, oracle, tmp_path, monkeypatch):
    """configs[0] at full scale (EPS_SYNTH_SCALE = 1: N = 4267, ~16 M rows): `--model simple` writes every candidate in the
    declared order; the truth is the dense float64 A @ A on the host -- scores AND (u, v) ids under the tie rule."""
    import argparse
    from eps_amd import datasets, filter_stage
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "1.0")
    fname = filter_stage.main(["--dataset", "ddi", "--model", "simple", "--checkpoint", "ddi_simple||0|0.pt", "--synthetic"])
    got = torch.load(fname)
    edge_index, edge_weight, _, data = datasets.get_data(argparse.Namespace(dataset="ddi", synthetic=True, use_feature=False))
    n = data.num_nodes
    assert n == 4267
    A = oracle.add_edges_scipy("ddi", edge_index.numpy(), edge_weight.numpy(), np.zeros((2, 0), np.int64), n)
    D = (A.toarray() != 0).astype(np.float64)
    C = D @ D
    np.fill_diagonal(C, 0.0)
    C[D != 0] = 0.0
    # column-major candidate order (filter.py:96-109): ascending (v, u); C is symmetric, so np.nonzero's (row, col) order is (v, u)
    v, u = np.nonzero(C)
    cn = C[v, u]
    del C
    order = oracle.sort_desc_stable(cn)
    assert got.dtype == torch.float32 and got.shape == (len(cn), 3), (tuple(got.shape), len(cn))
    assert len(cn) > 15_000_000
    g = got.numpy()
    assert np.array_equal(g[:, 2].astype(np.float64), cn[order]), "scores differ from the dense float64 A @ A"
    assert np.array_equal(g[:, 0].astype(np.int64), u[order]) and np.array_equal(g[:, 1].astype(np.int64), v[order]), \
        "(u, v) ids differ from the declared order"


def test_empty_column_list_reports_a_clean_status(eps, dev):
    """A launch of the piece kernel over NO columns (a rank whose list is empty) must hand the step a status word of 0: nothing
    clears it in the kernel then.  The list's small allocations come out of a fresh stream's pool whose only block was filled
    with 0xFF and freed, so a word nobody writes reads 0xFFFFFFFF."""
    from eps_amd import ops, scan, synth
    from eps_amd.heuristics import node_weight_table
    g = synth.rmat_graph(12, 8, 4, dev)
    w = node_weight_table(g, ops.W_AA)
    sc = scan.screen_weights(g, g, None, w)
    assert sc.usable
    fixw = scan.fixed_weights(g, w)
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        junk = torch.full((1 << 20,), -1, dtype=torch.int8, device=dev)     # (1 MiB: the largest block of the small pool)
        del junk
        for bar in (float("-inf"), 1.0):
            res = scan._launch(g, fixw, empty, bar, 1 << 20, both=True, screen=sc)
            slots, cand = res.counts()
            status = int(res.status.item())
            assert (slots, cand) == (0, 0)
            assert status == 0, f"status word {status & 0xFFFFFFFF:#x} of a launch over no columns"
    torch.cuda.synchronize()


def test_refine_keeps_sums_beyond_two_to_the_32(eps, dev):
    """eps_scan_refine completes a walked sum with its head term.  A sketch piece's estimate may lie anywhere below 2^32, so
    walked + head can exceed 2^32: a pair with s_walk = 2^32 - c / 2 and head term c must come out with score (s_walk + c) x
    2^-shift, not wrap to c / 2 and vanish.  Real eps_scan_heads / eps_scan_hub_rows tables, a hand-written walked list."""
    from eps_amd import ops
    from eps_amd.graph import CSRGraph
    n, hub = 64, 0
    edges = [(hub, x) for x in list(range(1, 41)) + [50, 51]] + [(50, 45), (50, 46), (51, 47)]
    ei = torch.tensor(edges, dtype=torch.int64).t()
    g = CSRGraph.from_edge_index(ei, None, sparse_sizes=(n, n)).to_symmetric().to(dev)
    f0, shift, bar = 1000, 20, 1000.0
    fx32 = torch.full((n,), f0, dtype=torch.int32, device=dev)
    heads = ops.scan_heads(g.rowptr, g.col, fx32, 1, f0)
    hubrows = ops.scan_hub_rows(g.rowptr, g.col, 1)
    hd = heads.cpu().numpy()
    assert hd[50].tolist() == [1, f0] and hd[51].tolist() == [1, f0]
    thr = int(bar * 2 ** shift)                   # (the kernel's bar in table units, to within one unit: no sum below lies that close)
    walked_sums = {(10, 50): 2 ** 32 - f0 // 2,   # head term f0 (10 is a neighbour of the hub): 2^32 + f0 / 2 in all
                   (11, 50): 2 ** 31 + 12345,     # bit 31 set: no known-edge flag here
                   (12, 51): thr - 5000,          # + f0: still below the bar
                   (13, 51): thr - 500,           # + f0: above it
                   (42, 50): 2 ** 32 - 1,         # no head term (42 is no neighbour of the hub): the largest walked sum
                   (43, 51): 100}
    adj = {}
    rp, col = g.rowptr.cpu().tolist(), g.col.cpu().tolist()
    for x in range(n):
        adj[x] = set(col[rp[x]:rp[x + 1]])
    want = {}
    for (u, v), s_walk in walked_sums.items():
        c = sum(f0 for w_ in col[rp[v]:rp[v] + int(hd[v][0])] if u in adj[w_])
        if s_walk + c >= thr:
            want[(u, v)] = float(np.float32(np.float32(np.uint64(s_walk + c)) * np.float32(2.0 ** -shift)))
    assert (10, 50) in want and (12, 51) not in want and (43, 51) not in want
    m = len(walked_sums)
    walked = ops.Survivors(16, 0.0, dev, prefill=False)
    walked.key[:m] = torch.tensor([(v << 32) | u for (u, v) in walked_sums], dtype=torch.int64, device=dev)
    walked.val.view(torch.int32)[:m] = torch.tensor(list(walked_sums.values()), dtype=torch.int64).to(torch.int32).to(dev)
    walked.rec[1:2].fill_(m)
    out = ops.Survivors(64, bar, dev, prefill=False)
    ops.scan_refine(walked, heads, hubrows, fx32, g.rowptr, g.col, n, shift, out)
    cnt = int(out.rec[1].item())
    keys, vals = out.key[:cnt].cpu().tolist(), out.val[:cnt].cpu().tolist()
    got = {(k & 0xFFFFFFFF, k >> 32): v for k, v in zip(keys, vals)}
    assert got == want

