"""GPU: the truncated-Katz pair kernel (csrc/katz_pairs.hip) against fp64 truth, the exact (inverse) branch, test_katz on the
reference's own fixtures, and rank.py --model katz end to end."""
import argparse
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

from conftest import golden_pair_files
from test_katz_host import (GRAPH_OF, LISTS, exact_tolerance, exact_truth, fixture_csr, load_fixture, truncated_truth)

pytestmark = pytest.mark.gpu

COEFFS = (0.05, 0.005, 0.000125)


def kernel_scores(eps, A, pairs, coeffs=COEFFS):
    """truncated_katz's kernel on a SciPy matrix (any shape of symmetry) and an [E,2] pair array -> float32 numpy."""
    from eps_amd import heuristics
    g = eps.CSRGraph.from_scipy(ssp.csr_matrix(A, dtype=np.float32), device="cuda:0")
    u = torch.from_numpy(np.ascontiguousarray(pairs[:, 0])).to(torch.int32).cuda()
    v = torch.from_numpy(np.ascontiguousarray(pairs[:, 1])).to(torch.int32).cuda()
    gt, p_out, p_in = heuristics._katz_transpose(g)
    out = eps.ops.katz_pair_scores(g.rowptr, g.col, g.val, gt.rowptr, gt.col, gt.val, p_out, p_in, g.n_rows, u, v, coeffs)
    return out.cpu().numpy()


def assert_within_one_ulp(got, truth, what=""):
    got = np.asarray(got, np.float64)
    ulp = np.spacing(np.abs(truth).astype(np.float32)).astype(np.float64)
    bad = np.abs(got - truth) > ulp
    assert not bad.any(), f"{what}: {int(bad.sum())} pairs off by more than one float32 ulp, e.g. {got[bad][:3]} vs {truth[bad][:3]}"


@pytest.mark.parametrize("path", golden_pair_files(), ids=lambda p: os.path.basename(p)[6:-4])
def test_kernel_matches_fp64_on_golden_graphs(eps, dev, path):
    d = np.load(path)
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((d["val"].astype(np.float64), d["col"], d["rowptr"]), shape=(n, n))
    pairs = d["pairs"].T.astype(np.int64)
    assert_within_one_ulp(kernel_scores(eps, A, pairs), truncated_truth(A, pairs, COEFFS), os.path.basename(path))


def directed_weighted(n=400, m=3000, seed=5):
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    A = ssp.coo_matrix((rng.integers(1, 7, m).astype(np.float64), (r, c)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    return A


def test_kernel_on_a_directed_weighted_matrix(eps, dev):
    """A is not symmetric: both (u,v) and (v,u) are scored and must come out as A's, not A^T's (a side swap shows here)."""
    A = directed_weighted()
    assert (A != A.T).nnz > 0
    rng = np.random.default_rng(1)
    coo = A.tocoo()
    stored = np.stack([coo.row, coo.col], 1)[:300]
    rand = rng.integers(0, A.shape[0], (700, 2))
    pairs = np.concatenate([stored, stored[:, ::-1], rand, rand[:, ::-1]])
    got = kernel_scores(eps, A, pairs)
    truth = truncated_truth(A, pairs, COEFFS)
    assert_within_one_ulp(got, truth, "directed")
    assert not np.allclose(truth, truncated_truth(A.T, pairs, COEFFS))         # the transpose would be a different answer


def hub_graph(weighted: bool):
    """Two hubs whose rows (and columns) hold far more entries than one wave's LDS map (1024), in a directed matrix, so both
    ends of a hub-hub pair search their map in global memory and the walks are long enough to be split over waves."""
    rng = np.random.default_rng(11)
    n = 6000
    r = np.concatenate([np.zeros(2500, int), rng.integers(0, n, 2500), np.ones(1800, int), rng.integers(0, n, 1800),
                        rng.integers(0, n, 20000)])
    c = np.concatenate([rng.integers(0, n, 2500), np.zeros(2500, int), rng.integers(0, n, 1800), np.ones(1800, int),
                        rng.integers(0, n, 20000)])
    w = rng.integers(1, 5, len(r)).astype(np.float64) if weighted else np.ones(len(r))
    A = ssp.coo_matrix((w, (r, c)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    if not weighted:
        A.data[:] = 1.0
    return A


@pytest.mark.parametrize("weighted", [False, True])
def test_kernel_on_hubs_beyond_the_lds_map(eps, dev, weighted):
    A = hub_graph(weighted)
    assert min(A[0].nnz, A[:, 0].nnz, A[1].nnz, A[:, 1].nnz) > 1024
    rng = np.random.default_rng(3)
    others = rng.integers(2, A.shape[0], 200)
    pairs = np.concatenate([[[0, 1], [1, 0], [0, 0], [1, 1]], np.stack([np.zeros(200, int), others], 1),
                            np.stack([others, np.ones(200, int)], 1), rng.integers(0, A.shape[0], (2000, 2))])
    assert_within_one_ulp(kernel_scores(eps, A, pairs), truncated_truth(A, pairs, COEFFS), "hubs")


def flat_walk_graph():
    """Directed, weighted, 98 nodes: nodes 0 and 1 point at the first 64 and at all 65 of the middle nodes 2 .. 66, middle node
    2 + i has (i + 1) % 4 entries among eight collectors 70 .. 77, every collector points at node 80, and eight feeders 90 .. 97
    point at every collector.  The walk of pair (0, 80) or (1, 80) is cheaper from the left end (the feeders make node 80's side
    dear) and short enough for one wave: one wave step of exactly 64 rows -- empty rows between rows of 1, 2 and 3 entries,
    96 entries in all -- and for node 1 a second step of one row."""
    rng = np.random.default_rng(64)
    mids, coll = np.arange(2, 67), np.arange(70, 78)
    e = [(0, m) for m in mids[:64]] + [(1, m) for m in mids]
    e += [(m, coll[(i + j) % 8]) for i, m in enumerate(mids) for j in range((i + 1) % 4)]
    e += [(c, 80) for c in coll] + [(f, c) for f in range(90, 98) for c in coll]
    r, c = zip(*e)
    return ssp.coo_matrix((rng.integers(1, 7, len(e)).astype(np.float64), (r, c)), shape=(98, 98)).tocsr()


def test_kernel_edge_cases(eps, dev):
    """Isolated nodes, u == v, pairs with no path of length <= 3 (exactly 0.0), and an empty list; then one wave step of exactly
    64 rows of the flattened walk, and 65 rows, with empty rows inside the step -- from either end of the pair."""
    F = flat_walk_graph()
    out_deg, in_deg = np.diff(F.indptr), np.diff(F.tocsc().indptr)
    p_out, p_in = (F != 0) @ out_deg, (F != 0).T @ in_deg               # the two-path counts the kernel plans with
    assert out_deg[0] == 64 and out_deg[1] == 65 and p_out[0] == 96 and p_out[1] == 97
    rows = out_deg[F[0].indices]
    assert rows[0] > 0 and rows[-2] > 0 and (rows == 0).sum() == 16
    for a in (0, 1):                                                    # walked from a (the cheaper end), by one wave
        assert p_out[a] + in_deg[80] <= p_in[80] + out_deg[a] and p_out[a] <= 2048
    fp = np.array([[0, 80], [1, 80], [0, 70], [1, 77], [0, 2], [1, 66], [90, 80], [0, 1], [80, 0]])
    ft = truncated_truth(F, fp, COEFFS)
    assert np.all(ft[:7] > 0) and np.all(ft[7:] == 0)
    assert_within_one_ulp(kernel_scores(eps, F, fp), ft, "flat walk, forward")
    assert_within_one_ulp(kernel_scores(eps, F.T.tocsr(), fp[:, ::-1]), ft, "flat walk, backward")
    # a path 0-1-2-3-4-5-6, a triangle 7-8-9, isolated 10, 11
    e = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (7, 8), (8, 9), (7, 9)]
    r, c = zip(*e)
    A = ssp.coo_matrix((np.ones(len(e)), (r, c)), shape=(12, 12)).tocsr()
    A = (A + A.T).tocsr()
    pairs = np.array([[10, 11], [10, 10], [0, 10], [0, 4], [0, 6], [0, 7], [0, 3], [0, 0], [7, 7], [2, 2], [8, 9], [3, 0]])
    got = kernel_scores(eps, A, pairs)
    truth = truncated_truth(A, pairs, COEFFS)
    assert_within_one_ulp(got, truth, "edge cases")
    assert np.all(got[:6] == 0.0) and np.all(got[6:] > 0)
    assert kernel_scores(eps, A, np.zeros((0, 2), np.int64)).shape == (0,)
    lib = eps.load()
    assert lib.eps_katz_pair_scores(None, None, None, None, None, None, None, None, 12, None, None, 0, *COEFFS, None, None,
                                    None) == 0


def test_kernel_is_deterministic(eps, dev):
    """Two launches over the same list are bitwise equal -- also for the pairs whose walks are split over several waves."""
    A = hub_graph(True)
    rng = np.random.default_rng(8)
    pairs = np.concatenate([np.stack([np.zeros(500, int), rng.integers(0, A.shape[0], 500)], 1),
                            rng.integers(0, A.shape[0], (20000, 2))])
    a = kernel_scores(eps, A, pairs)
    b = kernel_scores(eps, A, pairs)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- test_katz on the fixtures
def _fixture_data(eps, d):
    n = int(d["n"])
    g = {t: eps.CSRGraph.from_scipy(fixture_csr(d, t).astype(np.float32), device="cuda:0") for t in ("train", "full")}
    split = {"eval_train": {"edge": torch.from_numpy(d["pos_train_edge"])},
             "valid": {"edge": torch.from_numpy(d["pos_valid_edge"]), "edge_neg": torch.from_numpy(d["neg_valid_edge"])},
             "test": {"edge": torch.from_numpy(d["pos_test_edge"]), "edge_neg": torch.from_numpy(d["neg_test_edge"])}}
    data = argparse.Namespace(adj_t=g["train"], full_adj_t=g["full"] if str(d["dataset"]) == "collab" else g["train"],
                              num_nodes=n)
    return data, split


@pytest.mark.parametrize("name", ["katz_collab_like.npz", "katz_ddi_like.npz"])
def test_test_katz_matches_the_reference_fixture(eps, dev, name):
    from eps_amd import evaluate, heuristics
    d = load_fixture(name)
    dataset = str(d["dataset"])
    data, split = _fixture_data(eps, d)
    collab = dataset == "collab"
    score = heuristics.truncated_katz if collab else heuristics.exact_katz
    graphs = {"train": data.adj_t, "full": data.full_adj_t}
    H = None if collab else exact_truth(fixture_csr(d, "train"), float(d["beta"]))
    for lst in LISTS:
        got = score(graphs[GRAPH_OF[lst]], torch.from_numpy(d[f"{lst}_edge"]).t())
        ref = d[f"{lst}_pred"]
        assert got.dtype == (torch.float32 if collab else torch.float64) and got.numpy().dtype == ref.dtype
        if collab:
            den = np.maximum(np.abs(ref.astype(np.float64)), 1e-30)
            assert float((np.abs(got.numpy().astype(np.float64) - ref) / den).max()) <= 1e-5, lst
        else:
            assert float(np.abs(got.numpy() - ref).max()) <= exact_tolerance(float(d["cond"]), H), lst
    args = argparse.Namespace(dataset=dataset, model="katz")
    res = evaluate.test_katz(None, data, split, evaluate.evaluators[dataset], 64, args, dev)
    table = np.array([res[f"Hits@{K}"] for K in d["ks"]])
    assert np.array_equal(table, d["hits"]), (table, d["hits"])


# -------------------------------------------------------------------------------------------------- rank.py --model katz
def _host_katz(dataset, A, edges):
    A = A.astype(np.float64)
    if dataset == "collab":
        return truncated_truth(A, edges, COEFFS).astype(np.float32)
    A32 = (A.astype(np.float32) * np.float32(0.05)).astype(np.float64)         # beta*A in float32, as the reference forms it
    n = A.shape[0]
    H = np.linalg.inv(np.eye(n) - A32.toarray()) - np.eye(n)
    return H[edges[:, 0], edges[:, 1]]


def _hits(pos, neg, K):
    """ogb's Hits@K in the predictions' own dtype: kth = K-th largest negative; mean(pos > kth)."""
    neg = np.sort(np.asarray(neg))[::-1]
    return 1.0 if len(neg) < K else float(np.mean(np.asarray(pos) > neg[K - 1]))


@pytest.mark.parametrize("dataset,scale", [("collab", "0.004"), ("ddi", "0.02")])
def test_rank_cli_katz_matches_host_restatement(eps, oracle, tmp_path, monkeypatch, dataset, scale):
    """AA filter run -> rank.py --model katz at two sweep points (0 and k proposals): the curve points (Hits at the middle K on
    the validation and test lists) equal Hits of a host fp64 restatement on the same augmented graphs."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", scale)
    from eps_amd import datasets, evaluate, filter_stage, rank_stage
    filter_stage.main(["--dataset", dataset, "--model", "adamic_ogb", "--checkpoint", f"{dataset}_adamic_ogb||0|0.pt",
                       "--synthetic"])
    k = 200
    curves = rank_stage.main(["--dataset", dataset, "--model", "katz", "--sorted_edge_path",
                              f"{dataset}_adamic_ogb__0_0_sorted_edges.pt", "--sweep_num", "1", "--sweep_min", "0",
                              "--sweep_max", str(k), "--runs", "1", "--synthetic"])
    assert [c[0] for c in curves] == [0, k]
    edge_index, edge_weight, split_edge, data = datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True,
                                                                                     use_feature=False))
    props = torch.load(f"filtered_edges/{dataset}_adamic_ogb__0_0_sorted_edges.pt")
    K = evaluate.hits[dataset][1]
    n = data.num_nodes
    for curve, index_end in zip(curves, (0, k)):
        extra = props[:index_end, :2].t().long().numpy()
        A = oracle.add_edges_scipy(dataset, edge_index.numpy(), edge_weight.numpy(), extra, n)
        A_full = A
        if dataset == "collab":
            und = rank_stage.to_undirected(split_edge["valid"]["edge"].t()).numpy()
            A_full = oracle.add_edges_scipy(dataset, edge_index.numpy(), edge_weight.numpy(), np.concatenate([extra, und], 1), n)
        sc = lambda G, e: _host_katz(dataset, G, e.numpy())  # noqa: E731
        v = _hits(sc(A, split_edge["valid"]["edge"]), sc(A, split_edge["valid"]["edge_neg"]), K)
        t = _hits(sc(A_full, split_edge["test"]["edge"]), sc(A_full, split_edge["test"]["edge_neg"]), K)
        assert float(curve[1]) == pytest.approx(100 * v, abs=1e-4), (index_end, "valid")
        assert float(curve[2]) == pytest.approx(100 * t, abs=1e-4), (index_end, "test")


# ---------------------------------------------------------------------------------------------------------- full scale
def _full_data(dataset, monkeypatch):
    monkeypatch.delenv("EPS_SYNTH_SCALE", raising=False)
    from eps_amd import datasets
    return datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True, use_feature=False))


def test_full_scale_collab_kernel(eps, dev, monkeypatch):
    """The collab stand-in (N = 235,868): every test_katz list scored by the kernel; a seeded sample of 20 k pairs plus the
    100 longest walks checked against host fp64."""
    from eps_amd import heuristics
    edge_index, edge_weight, split_edge, data = _full_data("collab", monkeypatch)
    assert data.num_nodes == 235_868
    g = data.adj_t.to(dev)
    A = g.to_scipy().astype(np.float64)
    lists = [split_edge["eval_train"]["edge"], split_edge["valid"]["edge"], split_edge["valid"]["edge_neg"],
             split_edge["test"]["edge"], split_edge["test"]["edge_neg"]]
    pairs = torch.cat(lists).numpy().astype(np.int64)
    got = heuristics.truncated_katz(g, torch.from_numpy(pairs).t()).numpy()
    assert got.shape == (len(pairs),) and np.isfinite(got).all()
    _, p_out, p_in = heuristics._katz_transpose(g)
    po, pi = p_out.cpu().numpy(), p_in.cpu().numpy()
    deg = np.diff(A.indptr)
    u, v = pairs[:, 0], pairs[:, 1]
    walk = np.where(po[u] + deg[v] <= pi[v] + deg[u], po[u], pi[v])
    rng = np.random.default_rng(2024)
    idx = np.unique(np.concatenate([rng.choice(len(pairs), 20_000, replace=False), np.argsort(walk)[-100:]]))
    assert walk[idx].max() > 2048                                   # the split path is among the checked pairs
    assert_within_one_ulp(got[idx], truncated_truth(A, pairs[idx], COEFFS), "collab stand-in")


def test_full_scale_ddi_exact_branch(eps, dev, monkeypatch):
    """The ddi stand-in (N = 4267): the exact branch against numpy.linalg.inv, and the device inverse's residual."""
    from eps_amd import heuristics
    edge_index, edge_weight, split_edge, data = _full_data("ddi", monkeypatch)
    assert data.num_nodes == 4267
    g = data.adj_t.to(dev)
    pairs = torch.cat([split_edge["valid"]["edge"], split_edge["test"]["edge_neg"]])
    got = heuristics.exact_katz(g, pairs.t())
    assert got.dtype == torch.float64
    n = g.n_rows
    M = np.eye(n) - (g.to_scipy().astype(np.float32) * np.float32(0.05)).astype(np.float64).toarray()
    H_host = np.linalg.inv(M) - np.eye(n)
    e = pairs.numpy()
    ref = H_host[e[:, 0], e[:, 1]]
    cond = float(np.linalg.cond(M))
    assert float(np.abs(got.numpy() - ref).max()) <= 1e-15 * cond * max(1.0, float(np.abs(H_host).max())) * n
    H = heuristics._katz_inverse(g, 0.05)
    Md = torch.from_numpy(M).to(dev)
    resid = (Md @ (H + torch.eye(n, dtype=torch.float64, device=dev)) - torch.eye(n, dtype=torch.float64, device=dev))
    assert float(resid.abs().max()) <= 1e-8


def test_exact_branch_at_the_cap(eps, dev):
    """N = EXACT_KATZ_MAX_NODES still runs (three N x N float64 buffers at once: 6 GiB), with a small residual."""
    from eps_amd import heuristics
    n = heuristics.EXACT_KATZ_MAX_NODES
    rng = np.random.default_rng(4)
    r, c = rng.integers(0, n, 5 * n), rng.integers(0, n, 5 * n)
    A = ssp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float32).tocsr()
    g = eps.CSRGraph.from_scipy(A, device=dev)
    pairs = torch.from_numpy(rng.integers(0, n, (2, 1000)))
    got = heuristics.exact_katz(g, pairs)
    assert got.dtype == torch.float64 and got.shape == (1000,) and bool(torch.isfinite(got).all())
    H = heuristics._katz_inverse(g, 0.05)
    assert torch.equal(got, H[pairs[0].to(dev), pairs[1].to(dev)].cpu())
    row, col, _ = g.coo()
    M = torch.eye(n, dtype=torch.float64, device=dev)
    M[row, col] -= float(np.float32(0.05))
    resid = M @ (H + torch.eye(n, dtype=torch.float64, device=dev)) - torch.eye(n, dtype=torch.float64, device=dev)
    assert float(resid.abs().max()) <= 1e-8
