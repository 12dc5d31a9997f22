"""GPU: cosine-weighted common neighbours ('simplecos' / 'mlpcos').  The prologue kernels (csrc/cosine_cn.hip), the model
forward, the signed fused expansion, filter.py and rank.py end to end, and a sample of the full-size ppa-like graph -- all
against the float64 restatement of models.py:528-575 in test_cosine_cn_host.py."""
import argparse
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

from conftest import golden_pair_files
from test_cosine_cn_host import (all_pairs_sample, edge_cosines_truth, random_graph, raw_scores_truth, score_tolerance,
                                 scores_truth, smoothed_unit_features)

pytestmark = pytest.mark.gpu


def device_graph(eps, A):
    A = ssp.csr_matrix(A, dtype=np.float32)
    A.sort_indices()
    return eps.CSRGraph.from_scipy(A, device="cuda:0")


def directed_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    A = ssp.coo_matrix((rng.integers(1, 5, m).astype(np.float64), (rng.integers(0, n, m), rng.integers(0, n, m))),
                       shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def features(n, f, seed, ldx=None):
    """float32 [n, f] on the device, optionally a view with row stride ldx (unaligned rows take the scalar path)."""
    x = np.random.default_rng(seed).standard_normal((n, f)).astype(np.float32)
    x[1] = 0.0
    if ldx is None:
        return torch.from_numpy(x).cuda(), x
    buf = torch.zeros((n, ldx), dtype=torch.float32, device="cuda:0")
    buf[:, :f] = torch.from_numpy(x).cuda()
    return buf[:, :f], x


def check_prologue(eps, A, x_dev, x_np, use_revpos):
    from eps_amd import ops, scan
    g = device_graph(eps, A)
    f = x_np.shape[1]
    xhat = ops.cos_node_features(g.rowptr, g.col, g.val, x_dev)
    assert xhat.stride(0) % 32 == 0 and xhat.data_ptr() % 128 == 0
    truth = smoothed_unit_features(ssp.csr_matrix(A, dtype=np.float64), x_np.astype(np.float64))
    Ad = ssp.csr_matrix(abs(A), dtype=np.float64)
    deg = np.asarray(Ad.sum(1)).ravel() + 1e-6
    xp = x_np + (ssp.csr_matrix(A, dtype=np.float64) @ x_np) / deg[:, None]
    mag = (np.abs(x_np) + (Ad @ np.abs(x_np)) / deg[:, None]) / np.maximum(np.linalg.norm(xp, axis=1), 1e-8)[:, None]
    got = xhat.cpu().numpy()
    assert np.all(np.abs(got - truth) <= 1e-5 * (1 + f / 64) * (mag + 1e-3)), "xhat vs float64"
    pad = xhat.as_strided((g.n_rows, xhat.stride(0)), (xhat.stride(0), 1))[:, f:].cpu()
    assert bool((pad == 0).all()), "pad columns of xhat are zero"
    revpos = scan.reverse_positions(g) if use_revpos else None
    if use_revpos:
        assert scan.is_symmetric(g)
    c = ops.edge_cosines(g.rowptr, g.col, xhat, revpos).cpu().numpy()
    c_truth, c_mag = edge_cosines_truth(ssp.csr_matrix(A), truth)
    assert np.all(np.abs(c - c_truth) <= 1e-5 * (2 + f / 64) * (c_mag + 1e-3)), "edge cosines vs float64"
    return g, c


@pytest.mark.parametrize("f,ldx", [(1, None), (3, None), (58, None), (64, None), (128, None), (384, None), (1500, None),
                                   (2500, None), (61, 67), (600, 601)])
@pytest.mark.parametrize("kind", ["unit", "weighted", "directed"])
def test_prologue_kernels_vs_fp64(eps, dev, f, ldx, kind):
    if kind == "directed":
        A = directed_graph(300, 2500, seed=f)
    else:
        A = random_graph(300, 1500, seed=f, weighted=(kind == "weighted"), isolated=5)
        A = ssp.csr_matrix(A + ssp.diags(np.r_[np.zeros(297), np.ones(3)]))    # three self loops
    x_dev, x_np = features(A.shape[0], f, seed=f + 1, ldx=ldx)
    g, c = check_prologue(eps, A, x_dev, x_np, use_revpos=(kind != "directed"))
    if kind != "directed":               # the half computation + mirror writes equal the full one, bit for bit
        from eps_amd import ops
        xhat = ops.cos_node_features(g.rowptr, g.col, g.val, x_dev)
        full = ops.edge_cosines(g.rowptr, g.col, xhat, None).cpu().numpy()
        mirror = ssp.csr_matrix((c, A.indices, A.indptr), shape=A.shape)
        assert np.array_equal(c, full) or np.abs(c - full).max() <= 1e-6
        assert (abs(mirror - mirror.T) > 0).nnz == 0, "c is symmetric"


@pytest.mark.parametrize("path", golden_pair_files(), ids=lambda p: os.path.basename(p)[6:-4])
def test_prologue_and_scores_on_golden_graphs(eps, dev, path):
    d = np.load(path)
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((d["val"].astype(np.float64), d["col"], d["rowptr"]), shape=(n, n))
    x_dev, x_np = features(n, 58, seed=n)
    sym = (abs(A - A.T) > 0).nnz == 0
    check_prologue(eps, A, x_dev, x_np, use_revpos=sym)
    from eps_amd import heuristics
    got = heuristics.cosine_common_neighbors(device_graph(eps, A), x_dev, torch.from_numpy(d["pairs"]).long()).cpu().numpy()
    truth, mag = scores_truth(A, x_np.astype(np.float64), d["pairs"])
    assert np.all(np.abs(got - truth) <= score_tolerance(mag, 58))


def _model(model_type, n, f_in, hidden=None):
    from eps_amd import models
    emb = torch.nn.Embedding(n, hidden).cuda() if hidden else None
    return models.CommonNeighborsPredictor(emb, (hidden or 0) + f_in, hidden or 8, hidden or 8, 3, 0.0,
                                           model_type=model_type).cuda().eval()


@pytest.mark.parametrize("model_type", ["simplecos", "mlpcos"])
@pytest.mark.parametrize("weighted", [False, True])
def test_model_forward_vs_restatement(eps, dev, model_type, weighted):
    n = 500
    A = random_graph(n, 4000, seed=11, weighted=weighted, isolated=3)
    g = device_graph(eps, A)
    x_dev, x_np = features(n, 128, seed=2)
    hidden = 32 if model_type == "mlpcos" else None
    model = _model(model_type, n, 128, hidden)
    pairs = np.concatenate([all_pairs_sample(n, 3000, 5), np.array([[n - 1, 0], [n - 2, n - 1]])], 1)
    got = model(x_dev, torch.from_numpy(pairs), g).cpu().numpy()
    xin = x_np.astype(np.float64)
    if hidden:
        xin = np.concatenate([model.emb.weight.detach().cpu().numpy().astype(np.float64), xin], 1)
    truth, mag = scores_truth(A, xin, pairs)
    assert np.all(np.abs(got - truth) <= score_tolerance(mag, xin.shape[1]))
    assert got[-2] == 0.5 and got[-1] == 0.5
    if hidden:                                               # x is None: the embedding alone (models.py:529-530)
        got0 = model(None, torch.from_numpy(pairs), g).cpu().numpy()
        t0, m0 = scores_truth(A, model.emb.weight.detach().cpu().numpy().astype(np.float64), pairs)
        assert np.all(np.abs(got0 - t0) <= score_tolerance(m0, hidden))


def test_signed_expansion_keeps_negative_sums(eps, dev):
    """A graph whose common-neighbour sums are negative: the signed entry point returns them; the unsigned one takes a
    negative sum for a wrapped one and refuses (the guard the cosine path must not trip)."""
    from eps_amd import candidates, ops
    n = 200
    A = random_graph(n, 1500, seed=4)
    coo = A.tocoo()
    sign = np.where((coo.row < 100) == (coo.col < 100), 1.0, -1.0)          # symmetric signs
    S = ssp.csr_matrix((sign * 0.5, (coo.row, coo.col)), shape=A.shape)
    S.sort_indices()
    g = eps.CSRGraph(torch.from_numpy(S.indptr.astype(np.int64)).cuda(), torch.from_numpy(S.indices.astype(np.int32)).cuda(),
                     torch.from_numpy(S.data.astype(np.float32)).cuda(), n, n)
    ones = torch.ones(n, dtype=torch.float32, device="cuda:0")
    r = ops.expand_candidates(g.rowptr, g.col, g.val, ones, n, 0, n, want_cn=False, signed=True,
                              max_paths=candidates.max_paths_of(g))
    u, v, sc = r.pairs[0].long().cpu().numpy(), r.pairs[1].long().cpu().numpy(), r[4].cpu().numpy()
    truth = np.asarray(S[u].multiply(S[v]).sum(1)).ravel()
    assert (truth < 0).any()
    np.testing.assert_allclose(sc, truth, rtol=0, atol=1e-6)
    with pytest.raises(eps.EpsError, match="fixed-point"):
        ops.expand_candidates(g.rowptr, g.col, g.val, ones, n, 0, n, want_cn=False, max_paths=candidates.max_paths_of(g))


def _stand_in(dataset, scale, monkeypatch, model="simplecos"):
    monkeypatch.setenv("EPS_SYNTH_SCALE", scale)
    from eps_amd import datasets
    ei, ew, split_edge, data = datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True, use_feature=True))
    return ei, ew, split_edge, data


def test_fused_signed_path_equals_list_and_pair_path(eps, dev, monkeypatch):
    from eps_amd import candidates, filter_stage
    _, _, _, data = _stand_in("collab", "0.01", monkeypatch)
    data = data.to(torch.device("cuda:0"))
    model = _model("simplecos", data.num_nodes, data.x.shape[1])
    args = argparse.Namespace(model="simplecos")
    blocks = list(candidates.column_blocks(data.adj_t, max_paths=40_000))
    assert len(blocks) > 1
    got = {}
    for fused in (True, False):
        ps, ss = [], []
        for _, _, pairs, score in filter_stage.cosine_blocks(args, model, data, blocks, fused=fused):
            if isinstance(pairs, torch.Tensor):
                if pairs.shape[1]:
                    ps.append(pairs.long()), ss.append(score)
            else:
                idx = pairs.valid()
                ps.append(pairs.select(idx)), ss.append(score[idx])
        got[fused] = (torch.cat(ps, 1).cpu().numpy(), torch.cat(ss).cpu().numpy())
    assert np.array_equal(got[True][0], got[False][0]), "same candidates in the same order"
    assert np.abs(got[True][1] - got[False][1]).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------- CLIs
def _file_matches_truth(rows, A, x, n, keep):
    """rows: the proposal file [R,3]; every 2-hop non-edge of A is a candidate (filter.py:96-109), the truth is the
    float64 restatement, the order the declared rule (score descending, then candidate order).  Rows may differ from the
    truth's selection only inside the tolerance band at the K-th score."""
    from oracle import eps_oracle as orc
    cand, _ = orc.candidates_scipy(ssp.csr_matrix(A))                     # column-major: (u, v), keys ascending
    truth, mag = scores_truth(A, x, cand.T)
    tol = score_tolerance(mag, x.shape[1])
    key_all = cand[:, 1].astype(np.int64) * n + cand[:, 0]
    r = rows.numpy().astype(np.float64)
    key = r[:, 1].astype(np.int64) * n + r[:, 0].astype(np.int64)
    pos = np.searchsorted(key_all, key)
    assert np.array_equal(key_all[np.minimum(pos, key_all.size - 1)], key), "a proposal is not a candidate"
    assert np.unique(pos).size == pos.size
    sc = rows[:, 2].numpy()
    assert np.all(np.abs(sc - truth[pos]) <= tol[pos]), "scores vs float64"
    assert np.all(sc[:-1] >= sc[1:]), "scores descending"
    ties = sc[:-1] == sc[1:]
    assert np.all(pos[:-1][ties] < pos[1:][ties]), "equal scores in candidate order"
    if not keep:
        assert pos.size == key_all.size, "the whole candidate set"
        return sc
    assert pos.size == min(keep, key_all.size)
    kth = float(sc[-1])
    out = np.ones(key_all.size, bool)
    out[pos] = False
    assert np.all(truth[out] - tol[out] <= kth), "a candidate above the K-th score is missing"
    return sc


def _planted_ppa(tmp_path, monkeypatch):
    """The small ppa stand-in with a planted complete bipartite block K(30, 40) of nodes of one feature class: its same-side
    pairs are candidates with ~40 common neighbours of cosine ~1, raw sums far above 17.3, so their float32 sigmoid is
    exactly 1.0 -- the saturated bar of the full-size graph's hubs, on a graph small enough for a float64 truth of every
    candidate.  Written as a dataset file ($EPS_DATA_ROOT/ppa.pt)."""
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.004")
    from eps_amd import datasets
    raw = datasets.load_raw("ppa", synthetic=True)
    n = int(raw["num_nodes"])
    nodes = torch.from_numpy(np.random.default_rng(0).choice(n, 70, replace=False))
    left, right = nodes[:30], nodes[30:]
    block = torch.stack([left.repeat_interleave(40), right.repeat(30)])
    ei = torch.cat([raw["edge_index"], block, block.flip(0)], 1)
    key = torch.unique(ei[0] * n + ei[1])                           # (planted edges the stand-in already had: once)
    raw["edge_index"] = torch.stack([key // n, key % n])
    raw["x"][nodes] = 0.0
    raw["x"][nodes, 0] = 1.0
    torch.save(raw, tmp_path / "ppa.pt")
    monkeypatch.setenv("EPS_DATA_ROOT", str(tmp_path))
    return datasets.get_data(argparse.Namespace(dataset="ppa", synthetic=False, use_feature=True))


def _many_blocks(monkeypatch, A, n_blocks=12):
    """Split the filter's candidate generation into about ``n_blocks`` column blocks (the two-hop paths of the graph are
    sum_w deg(w)^2), so that a --keep_top run reads the streaming top-K's bar before most blocks -- the in-kernel cut."""
    from eps_amd import candidates
    deg = np.diff(ssp.csr_matrix(A).indptr).astype(np.int64)
    monkeypatch.setattr(candidates, "DEFAULT_BLOCK_PATHS", max(int((deg * deg).sum()) // n_blocks, 1))


def _cut_kinds():
    """What the last fused cosine run did per column block: {"scored" / "cut" / "skipped": [raw thresholds]}."""
    from eps_amd import filter_stage
    kinds = {}
    for _, _, thr, kind in filter_stage.LAST_COSINE_CUTS:
        kinds.setdefault(kind, []).append(thr)
    return kinds


@pytest.mark.parametrize("dataset", ["collab", "ppa"])
def test_filter_cli_simplecos(eps, oracle, dev, tmp_path, monkeypatch, dataset):
    """The whole file (--keep_top 0) and --keep_top K -- on ppa also at a K whose bar saturates at 1.0 -- against the float64
    restatement under the tie rule, over a dozen column blocks: after the first blocks the kernel's cut runs at a finite raw
    threshold, and once the bar is 1.0 the remaining columns are skipped."""
    monkeypatch.chdir(tmp_path)
    if dataset == "ppa":
        ei, ew, _, data = _planted_ppa(tmp_path, monkeypatch)
        synthetic = []
    else:
        ei, ew, _, data = _stand_in(dataset, "0.01", monkeypatch)
        synthetic = ["--synthetic"]
    from eps_amd import filter_stage
    A = oracle.add_edges_scipy(dataset, ei.numpy(), ew.numpy(), np.zeros((2, 0), np.int64), data.num_nodes)
    _many_blocks(monkeypatch, A)
    argv = ["--dataset", dataset, "--model", "simplecos", "--checkpoint", f"{dataset}_simplecos||0|0.pt",
            "--use_feature", "True"] + synthetic
    full = torch.load(filter_stage.main(argv))
    kinds = _cut_kinds()
    assert set(kinds) == {"scored"} and len(kinds["scored"]) >= 8, "the whole file: every block scored in full"
    x = data.x.numpy().astype(np.float64)
    sc = _file_matches_truth(full, A, x, data.num_nodes, 0)
    n_sat = int((sc == 1.0).sum())
    ks = [1000]
    if dataset == "ppa":
        assert n_sat >= 2 * 30 * 29, "the planted block saturates sigmoid at 1.0f"
        ks.append(n_sat // 2)
    for k in ks:
        top = torch.load(filter_stage.main(argv[:5] + [f"{dataset}_simplecos||0|{k}.pt"] + argv[6:] + ["--keep_top", str(k)]))
        kinds = _cut_kinds()
        assert len(kinds.get("cut", [])) >= 2 and all(np.isfinite(t) for t in kinds["cut"]), kinds
        _file_matches_truth(top, A, x, data.num_nodes, k)
        assert torch.equal(top, full[:k]), "--keep_top K == the first K rows of the whole file"
        if k != 1000:
            assert float(top[-1, 2]) == 1.0
            assert kinds.get("skipped") == [float("inf")], "the saturated bar ends the expansion"


def test_filter_cli_mlpcos_loads_a_reference_state_dict(eps, oracle, dev, tmp_path, monkeypatch):
    """A state dict with the reference's keys (mlp.lins.*, emb.weight: the restated constructor, models.py:136-163 and
    :513-517) loads, and the scores are those of [emb.weight || x]."""
    monkeypatch.chdir(tmp_path)
    ei, ew, _, data = _stand_in("collab", "0.01", monkeypatch)
    n, hidden = data.num_nodes, 256
    torch.manual_seed(3)
    ref = torch.nn.Module()
    ref.mlp = torch.nn.Module()
    ref.mlp.lins = torch.nn.ModuleList([torch.nn.Linear(hidden + 128, hidden), torch.nn.Linear(hidden, hidden),
                                        torch.nn.Linear(hidden, hidden)])
    ref.emb = torch.nn.Embedding(n, hidden)
    os.makedirs("models")
    torch.save(ref.state_dict(), "models/collab_mlpcos||0|0.pt")
    from eps_amd import filter_stage
    A = oracle.add_edges_scipy("collab", ei.numpy(), ew.numpy(), np.zeros((2, 0), np.int64), n)
    _many_blocks(monkeypatch, A)
    rows = torch.load(filter_stage.main(["--dataset", "collab", "--model", "mlpcos", "--checkpoint", "collab_mlpcos||0|0.pt",
                                         "--synthetic", "--keep_top", "2000"]))
    assert len(_cut_kinds().get("cut", [])) >= 2
    x = np.concatenate([ref.emb.weight.detach().numpy(), data.x.numpy()], 1).astype(np.float64)
    _file_matches_truth(rows, A, x, n, 2000)


def _hits_band(pos, neg, K):
    """(lowest, highest) Hits@K the float64 scores allow when every score may move inside its tolerance."""
    (p, pt), (q, qt) = pos, neg
    if len(q) < K:
        return 1.0, 1.0
    kth_hi = np.sort(q + qt)[-K]
    kth_lo = np.sort(q - qt)[-K]
    return float(np.mean(p - pt > kth_hi)), float(np.mean(p + pt > kth_lo))


@pytest.mark.parametrize("model", ["simplecos", "mlpcos"])
def test_rank_cli_cosine_hits(eps, oracle, dev, tmp_path, monkeypatch, model):
    """rank.py --model simplecos (no parameters, evaluated like the reference) and --model mlpcos --load_model (a reference
    state dict, evaluated without training): Hits at the middle K vs the float64 restatement at two sweep points."""
    monkeypatch.chdir(tmp_path)
    dataset = "collab"
    ei, ew, split_edge, data = _stand_in(dataset, "0.02", monkeypatch)
    from eps_amd import evaluate, filter_stage, rank_stage
    filter_stage.main(["--dataset", dataset, "--model", "adamic_ogb", "--checkpoint", f"{dataset}_adamic_ogb||0|0.pt",
                       "--synthetic"])
    n, x = data.num_nodes, data.x.numpy().astype(np.float64)
    extra_argv = []
    if model == "mlpcos":
        hidden = 256                                    # collab's mlpcos row: 3 layers of 256, embedding + 128 features
        torch.manual_seed(5)
        ref = torch.nn.Module()
        ref.mlp = torch.nn.Module()
        ref.mlp.lins = torch.nn.ModuleList([torch.nn.Linear(hidden + 128, hidden), torch.nn.Linear(hidden, hidden),
                                            torch.nn.Linear(hidden, hidden)])
        ref.emb = torch.nn.Embedding(n, hidden)
        torch.save(ref.state_dict(), "mlpcos_ref.pt")
        extra_argv = ["--load_model", "mlpcos_ref.pt"]
        x = np.concatenate([ref.emb.weight.detach().numpy().astype(np.float64), x], 1)
    k = 200
    curves = rank_stage.main(["--dataset", dataset, "--model", model, "--sorted_edge_path",
                              f"{dataset}_adamic_ogb__0_0_sorted_edges.pt", "--sweep_num", "1", "--sweep_min", "0",
                              "--sweep_max", str(k), "--runs", "1", "--synthetic"] + extra_argv)
    assert [c[0] for c in curves] == [0, k]
    props = torch.load(f"filtered_edges/{dataset}_adamic_ogb__0_0_sorted_edges.pt")
    K = evaluate.hits[dataset][1]
    for curve, index_end in zip(curves, (0, k)):
        extra = props[:index_end, :2].t().long().numpy()
        A = oracle.add_edges_scipy(dataset, ei.numpy(), ew.numpy(), extra, n)
        und = rank_stage.to_undirected(split_edge["valid"]["edge"].t()).numpy()
        A_full = oracle.add_edges_scipy(dataset, ei.numpy(), ew.numpy(), np.concatenate([extra, und], 1), n)

        def sc(G, e):
            s, mag = scores_truth(G, x, e.t().numpy())
            return s, score_tolerance(mag, x.shape[1])
        lo, hi = _hits_band(sc(A, split_edge["valid"]["edge"]), sc(A, split_edge["valid"]["edge_neg"]), K)
        assert 100 * lo - 1e-4 <= float(curve[1]) <= 100 * hi + 1e-4, (index_end, "valid", lo, hi)
        lo, hi = _hits_band(sc(A_full, split_edge["test"]["edge"]), sc(A_full, split_edge["test"]["edge_neg"]), K)
        assert 100 * lo - 1e-4 <= float(curve[2]) <= 100 * hi + 1e-4, (index_end, "test", lo, hi)


# ---------------------------------------------------------------------------------------------------------- full size
def test_full_size_ppa_sample(eps, dev, monkeypatch):
    """The cosine graph of the full-size ppa-like stand-in (576 k nodes, 54 M stored entries): a seeded sample of entries
    and of pairs (random and two-hop) against float64."""
    monkeypatch.delenv("EPS_SYNTH_SCALE", raising=False)
    from eps_amd import datasets, heuristics
    _, _, _, data = datasets.get_data(argparse.Namespace(dataset="ppa", synthetic=True, use_feature=True))
    data = data.to(torch.device("cuda:0"))
    g = data.adj_t
    gc = heuristics.cosine_graph(g, data.x)
    A = g.to_scipy().tocsr()
    A.sort_indices()
    x = data.x.cpu().numpy().astype(np.float64)
    xhat = smoothed_unit_features(A, x)
    rng = np.random.default_rng(0)
    e = rng.integers(0, A.nnz, 20000)
    row = np.searchsorted(A.indptr, e, side="right") - 1
    prod = xhat[row] * xhat[A.indices[e]]
    c = gc.val.cpu().numpy()[e]
    assert np.all(np.abs(c - prod.sum(1)) <= 1e-5 * (2 + 58 / 64) * (np.abs(prod).sum(1) + 1e-3))
    n = A.shape[0]
    u = rng.integers(0, n, 3000)
    w = A.indices[A.indptr[u] + rng.integers(0, 1 << 30, 3000) % np.maximum(np.diff(A.indptr)[u], 1)]
    v = A.indices[A.indptr[w] + rng.integers(0, 1 << 30, 3000) % np.maximum(np.diff(A.indptr)[w], 1)]
    pairs = np.concatenate([np.stack([u, v]), all_pairs_sample(n, 3000, 9)], 1)
    got = heuristics.cosine_common_neighbors(g, data.x, torch.from_numpy(pairs)).cpu().numpy()
    # truth from the sampled rows only (a full host C would be 54 M x 58 products)
    raw = np.zeros(pairs.shape[1])
    mag = np.zeros(pairs.shape[1])
    for i, (a, b) in enumerate(pairs.T):
        ws = np.intersect1d(A.indices[A.indptr[a]:A.indptr[a + 1]], A.indices[A.indptr[b]:A.indptr[b + 1]])
        if ws.size:
            t = (xhat[ws] @ xhat[a]) * (xhat[ws] @ xhat[b])
            raw[i], mag[i] = t.sum(), np.abs(t).sum()
    truth = 1.0 / (1.0 + np.exp(-raw))
    assert np.all(np.abs(got - truth) <= score_tolerance(mag, 58))
    assert (raw > 0).sum() > 1000
