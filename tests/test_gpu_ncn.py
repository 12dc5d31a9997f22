"""GPU: models.cn_embed_sum (forward and backward, bit for bit against sequential float32 sums), the NCN models' gradients
against the float64 restatement of tests/cn_list_truth.py under the rules of tests/test_gpu_training.py, the symmetry of the
scores, and rank.py / filter.py --model ncn through their command lines."""
import argparse
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import cn_list_truth as ct
import test_gpu_training as tgt
import training_truth as tt

pytestmark = pytest.mark.gpu

WIDTHS = [1, 58, 64, 256, 260]                   # the scalar SpMM kernel (1, 58), the float4 kernel, a second column pass (260)
H_MAX = max(WIDTHS)


def _graph(eps, A, dev):
    A = ssp.csr_matrix(A, dtype=np.float32)
    A.sort_indices()
    return eps.CSRGraph.from_scipy(A, device=dev)


@pytest.fixture(scope="module")
def cases(eps, dev):
    """Two lists with their truths, computed once at the widest H (a sum is column-wise: a narrower h is a column slice):
    the boundary graph's pairs, and stored edges + uniform pairs of a 2048-node R-MAT graph."""
    from eps_amd import ops, synth
    out = {}
    cap, ratio = ops.pair_cn_list_limits()
    A, special, stranger = ct.boundary_graph(cap, ratio)
    u, v = ct.boundary_pairs(A, special, stranger)
    out["boundary"] = (A, u, v)
    R = ssp.csr_matrix(synth.rmat_graph(11, 8, 7, "cpu").to_scipy().astype(np.float32))
    coo, rng = R.tocoo(), np.random.default_rng(9)
    pick = rng.integers(0, coo.nnz, 2048)
    neg = rng.integers(0, R.shape[0], (2, 2048))
    out["rmat"] = (R, np.concatenate([coo.row[pick], neg[0]]).astype(np.int32), np.concatenate([coo.col[pick], neg[1]]).astype(np.int32))
    res = {}
    for name, (A, u, v) in out.items():
        n = A.shape[0]
        rng = np.random.default_rng(12)
        h = rng.standard_normal((n, H_MAX)).astype(np.float32)
        dz = rng.standard_normal((len(u), H_MAX)).astype(np.float32)
        ptr, w = ct.cn_lists(A, u, v)
        tptr, tb = ct.transpose_stable(ptr, w, n)
        z64, zabs = ct.sum_f64(ptr, w, h, n)
        d64, dabs = ct.sum_f64(tptr, tb, dz, len(u))
        res[name] = dict(adj=_graph(eps, A, dev), n=n, edges=torch.from_numpy(np.stack([u, v]).astype(np.int64)).to(dev),
                         h=h, dz=dz, ptr=ptr, w=w, tptr=tptr, z32=ct.seq_sum_f32(ptr, w, h), z64=z64, zabs=zabs,
                         d32=ct.seq_sum_f32(tptr, tb, dz), d64=d64, dabs=dabs)
    return res


def _within_gamma(got, ref64, refabs, counts):
    bound = ct.gamma(counts)[:, None] * refabs
    err = np.abs(got.astype(np.float64) - ref64)
    return bool((err <= bound).all())


@pytest.mark.parametrize("name", ["boundary", "rmat"])
@pytest.mark.parametrize("H", WIDTHS)
def test_cn_embed_sum_forward(eps, dev, cases, monkeypatch, name, H):
    from eps_amd import models
    c = cases[name]
    h = torch.from_numpy(np.ascontiguousarray(c["h"][:, :H])).to(dev)
    with torch.no_grad():
        z = models.cn_embed_sum(h, c["adj"], c["edges"])
    assert z.shape == (c["edges"].shape[1], H) and z.dtype == torch.float32
    got = z.cpu().numpy()
    assert got.tobytes() == np.ascontiguousarray(c["z32"][:, :H]).tobytes()            # the sequential float32 sum, bit for bit
    assert _within_gamma(got, c["z64"][:, :H], c["zabs"][:, :H], np.diff(c["ptr"]))
    # the budget cuts the batch, not the sums: under no_grad and with autograd recording
    monkeypatch.setattr(models, "CN_LIST_BUDGET", 1000)
    assert int(np.diff(c["ptr"]).max()) > 1000 or name == "rmat"                       # (a single pair beyond the budget, too)
    with torch.no_grad():
        z2 = models.cn_embed_sum(h, c["adj"], c["edges"])
    assert torch.equal(z2, z)
    if H == 64:
        z3 = models.cn_embed_sum(h.clone().requires_grad_(True), c["adj"], c["edges"])
        assert z3.requires_grad and torch.equal(z3.detach(), z)


@pytest.mark.parametrize("name", ["boundary", "rmat"])
@pytest.mark.parametrize("H", [58, 256])
def test_cn_embed_sum_backward(eps, dev, cases, name, H):
    from eps_amd import models
    c = cases[name]
    dz = torch.from_numpy(np.ascontiguousarray(c["dz"][:, :H])).to(dev)
    grads = []
    for _ in range(2):
        h = torch.from_numpy(np.ascontiguousarray(c["h"][:, :H])).to(dev).requires_grad_(True)
        models.cn_embed_sum(h, c["adj"], c["edges"]).backward(dz)
        grads.append(h.grad)
    assert torch.equal(grads[0], grads[1])                                             # two runs, the same bits
    got = grads[0].cpu().numpy()
    assert got.shape == (c["n"], H)
    assert got.tobytes() == np.ascontiguousarray(c["d32"][:, :H]).tobytes()            # sequential in ascending b, bit for bit
    listed = np.diff(c["tptr"])
    assert _within_gamma(got, c["d64"][:, :H], c["dabs"][:, :H], listed)
    assert (listed == 0).any() and not got[listed == 0].any()                          # no pair's common neighbour: exact zeros
    # no gradient wanted: nothing is transposed, nothing comes back
    h = torch.from_numpy(np.ascontiguousarray(c["h"][:, :H])).to(dev)
    assert not models.cn_embed_sum(h, c["adj"], c["edges"]).requires_grad


# ---------------------------------------------------------------------------------------------------------- model gradients
LAST_SCORE_RATIOS = {}


@pytest.mark.parametrize("encoder", ["gcn", "sage"])
@pytest.mark.parametrize("kind", ["unit", "weighted"])
@pytest.mark.parametrize("H", [64, 256])
def test_model_gradients(eps, dev, encoder, kind, H):
    """NCNLinkGNN (3 layers, dropout 0) on a 2048-node R-MAT graph: every parameter's gradient and the train-mode scores against
    the float64 restatement, under the rules of test_gpu_training.test_model_gradients_at_dataset_shapes.  The scores are held
    to max(1e-5, 4 x the float32 dense formulation's own distance from float64): z_cn is a longer sum than anything in the
    GCN decoder, so the plain 1e-5 is not assumed."""
    from eps_amd import models
    adj = tgt._model_graph(kind, 11, dev, eps)
    n = adj.n_rows
    torch.manual_seed(3)
    cls = models.GCN if encoder == "gcn" else models.SAGE
    model = models.NCNLinkGNN(torch.nn.Embedding(n, H), cls(H, H, H, 3, 0.0), models.NCNPredictor(H, H, 1, 3, 0.0)).to(dev)
    model.train()
    gen = torch.Generator().manual_seed(4)
    n_pos = 2048
    edges = tgt._edge_batch(adj, n_pos, gen).to(dev)
    taken = []
    lp = model.linkpred
    hooks = [m.register_forward_hook(lambda mod, inp, o: taken.append(o.detach() > 0))
             for m in list(model.gnn.convs[:-1]) + [lp.xij_lin, lp.xcn_lin] + list(lp.lins[:-1])]
    out = model(None, edges, adj).squeeze(1)
    for hk in hooks:
        hk.remove()
    tt.log_loss(out, n_pos).backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values()) and len(taken) == 5
    pre = []
    with torch.no_grad():
        ct.ncn_forward(encoder, tt.params_as(model, torch.float64), tt.dense_adjacency(adj, torch.float64, dev),
                       tt.dense_pattern(adj, torch.float64, dev), None, edges, pre=pre)
    flips = 0
    for z, mask in zip(pre, taken):
        differ = (z > 0) != mask
        flips += int(differ.sum())
        assert float(z[differ].abs().max()) <= 1e-5 * max(1.0, float(z.abs().max())) if bool(differ.any()) else True
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = tt.params_as(model, dt)
        A, P = tt.dense_adjacency(adj, dt, dev), tt.dense_pattern(adj, dt, dev)
        o = ct.ncn_forward(encoder, p, A, P, None, edges, branch=taken)
        tt.log_loss(o, n_pos).backward()
        ref[dt] = (o.detach(), {k: v.grad for k, v in p.items()})
    out_err = float((out.detach().double() - ref[torch.float64][0]).abs().max())
    f32_err = float((ref[torch.float32][0].double() - ref[torch.float64][0]).abs().max())
    tag = f"ncn {encoder}/{kind}/H={H}"
    LAST_SCORE_RATIOS[tag] = out_err / max(1e-5, 4.0 * f32_err)
    print(f"\n{tag}: ReLU inputs whose sign differs between the HIP forward and float64: {flips}; train-mode scores, "
          f"max |hip - f64| = {out_err:.3g}, f32 dense: {f32_err:.3g}, ratio to max(1e-5, 4 x f32 dense) = {LAST_SCORE_RATIOS[tag]:.3f}")
    assert out_err <= max(1e-5, 4.0 * f32_err)
    tgt._check_grads(tag, grads, ref[torch.float64][1], ref[torch.float32][1], floor=1e-6)


# ---------------------------------------------------------------------------------------------------------- symmetry
def test_scores_are_symmetric_bit_for_bit(eps, dev):
    from eps_amd import models
    adj = tgt._model_graph("weighted", 11, dev, eps)
    n, H = adj.n_rows, 64
    torch.manual_seed(5)
    model = models.NCNLinkGNN(torch.nn.Embedding(n, H), models.GCN(H, H, H, 2, 0.0), models.NCNPredictor(H, H, 1, 2, 0.0)).to(dev)
    model.eval()
    e = torch.randint(0, n, (2, 10_000), generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        a = model(None, e, adj)
        b = model(None, e.flip(0), adj)
        assert a.shape == (10_000, 1) and torch.equal(a, b) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
        assert len(torch.unique(a)) > 1000
        # a pair's score does not depend on the batch it arrives in
        c = torch.cat([model(None, e[:, :3001], adj), model(None, e[:, 3001:], adj)])
        assert torch.equal(c, a)


# ---------------------------------------------------------------------------------------------------------- command lines
@pytest.fixture(scope="module")
def trained(eps, dev, tmp_path_factory):
    """rank.py --dataset ddi --model ncn --synthetic on the 0.08 stand-in, once: the directory it ran in (models/, curves/), its
    losses and its curve."""
    from eps_amd import rank_stage, training
    work = tmp_path_factory.mktemp("ncn_cli")
    mp = pytest.MonkeyPatch()
    try:
        mp.chdir(work)
        mp.setenv("EPS_SYNTH_SCALE", "0.08")
        losses = []
        orig = training.train

        def spy(*a, **k):
            losses.append(orig(*a, **k))
            return losses[-1]

        mp.setattr(rank_stage, "train", spy)
        torch.manual_seed(1)
        curves = rank_stage.main(["--dataset", "ddi", "--model", "ncn", "--synthetic", "--hidden_channels", "32", "--epochs", "12",
                                  "--runs", "1", "--batch_size", "4096", "--save_models", "--eval_steps", "4"])
    finally:
        mp.undo()
    return dict(dir=work, losses=losses, curves=curves)


def test_rank_cli_trains_ncn(trained):
    losses = trained["losses"]
    print(f"\nrank.py --model ncn: losses {losses}")
    assert len(losses) == 12 and all(np.isfinite(losses)) and min(losses[-3:]) < losses[0], losses
    curves = trained["curves"]
    assert len(curves) == 1 and 0.0 <= float(curves[0][1]) <= 100.0 and 0.0 <= float(curves[0][2]) <= 100.0
    assert [f for f in os.listdir(trained["dir"] / "models") if f.startswith("ddi_ncn")] == ["ddi_ncn||0|0.pt"]


def test_filter_cli_equals_the_restatement(eps, dev, trained, monkeypatch):
    """filter.py --model ncn with the trained checkpoint: --keep_top 1000 (the half-list route, and the same with small candidate
    blocks) and --keep_per_node 3 against the filter restated here -- every candidate expanded, scored by the model's forward
    in ONE call, ordered by the declared rule.  Exact on the pairs, bit-exact on the scores."""
    monkeypatch.chdir(trained["dir"])
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.08")
    from eps_amd import candidates, datasets, filter_stage, graph, models, proposals
    argv = ["--dataset", "ddi", "--model", "ncn", "--checkpoint", "ddi_ncn||0|0.pt", "--synthetic", "--hidden_channels", "32"]
    args = models.default_model_configs(filter_stage.make_parser().parse_args(argv))
    ei, ew, _, data = datasets.get_data(args)
    data = data.to(dev)
    model = models.build_model(args, data, dev)
    model.load_state_dict(torch.load("models/ddi_ncn||0|0.pt", map_location=dev))
    model.eval()
    adj = graph.add_edges("ddi", ei.to(dev), ew.to(dev), torch.zeros((2, 0), dtype=torch.long, device=dev), data.num_nodes)
    with torch.no_grad():
        pairs = candidates.expand_block(adj, 0, adj.n_rows)[0]
        score = model(data.x, pairs, adj).reshape(-1)
        full = proposals.sorted_edges_tensor(pairs, score).cpu()
        pos = filter_stage.per_node_positions(pairs, score, 0, adj.n_rows, 3)
        per_node = proposals.sorted_edges_tensor(pairs[:, pos], score[pos]).cpu()
    assert full.shape[0] > 5000 and len(torch.unique(full[:, 2])) > 1000

    got = torch.load(filter_stage.main(argv + ["--keep_top", "1000"]))
    assert got.shape == (1000, 3) and got.dtype == torch.float32 and torch.equal(got, full[:1000])
    assert torch.equal(torch.load(filter_stage.main(argv)), full)                      # no cut: the whole file
    with pytest.raises(ValueError, match="no MLP decode"):
        filter_stage.main(argv + ["--keep_top", "1000", "--decode_precision", "bf16"])
    monkeypatch.setattr(candidates, "DEFAULT_BLOCK_PATHS", 20_000)                     # many small candidate blocks
    assert torch.equal(torch.load(filter_stage.main(argv + ["--keep_top", "1000"])), full[:1000])
    got = torch.load(filter_stage.main(argv + ["--keep_per_node", "3"]))
    assert torch.equal(got, per_node)
