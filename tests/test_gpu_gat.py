"""GPU: the graph-attention kernels (csrc/gat_attend.hip) and what is built on them -- ops.gat_aggregate and
ops.gat_aggregate_backward against the float64 truth of tests/gat_truth.py within its per-element bounds, their reproducibility bit
for bit, models.GATConv in train and eval mode, a GAT LinkGNN's parameter gradients against float64 autograd, and the command
lines (rank.py / filter.py --model gat, the row-sharded last layer)."""
import os

import numpy as np
import pytest
import torch

import gat_truth as gt
import test_gpu_training as tgt
import training_truth as tt

pytestmark = pytest.mark.gpu

RATIOS = {}          # the largest error / bound per quantity, printed by the tests that measure them


def _dev_case(c, dev):
    t = lambda a: torch.from_numpy(a).to(dev)
    return dict(rowptr=t(c["rowptr"]), col=t(c["col"]), z=t(c["z"]), s_src=t(c["s_src"]), s_dst=t(c["s_dst"]), bias=t(c["bias"]),
                gout=t(c["gout"]))


def _ratio(tag, got, want, bound):
    r = float((np.abs(got.double().cpu().numpy() - want) / np.maximum(bound, 1e-300)).max())
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), r)
    return r


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("regime", gt.REGIMES)
@pytest.mark.parametrize("f,heads", gt.SHAPES)
def test_forward_within_the_bound(eps, dev, f, heads, regime):
    """ops.gat_aggregate on every (shape, regime) of the row-length graph, with and without bias and ReLU: every element inside
    the forward bound, lse inside its own, every output finite (regime "wide": an exp without the max subtracted overflows)."""
    from eps_amd import ops
    d = _dev_case(gt.case(f, heads, regime), dev)
    for bias, relu in ((False, False), (True, False), (True, True)):
        tr = gt.forward_truth(f, heads, regime, bias, relu)
        out, lse = ops.gat_aggregate(d["rowptr"], d["col"], d["z"], d["s_src"], d["s_dst"], heads, bias=d["bias"] if bias else None,
                                     relu=relu, want_lse=True)
        assert out.shape == (gt.N_NODES, f) and lse.shape == (gt.N_NODES, heads)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
        r_out = _ratio("forward", out, tr["out"], tr["bound"])
        r_lse = _ratio("lse", lse, tr["lse"], tr["lse_bound"])
        print(f"\nf={f} heads={heads} {regime} bias={bias} relu={relu}: largest error / bound: out {r_out:.3f}, lse {r_lse:.3f}")
        assert r_out <= 1.0 and r_lse <= 1.0
    print(f"\nlargest device error / bound so far: {RATIOS}")


@pytest.mark.parametrize("f,heads", [(64, 8), (300, 3)])
def test_same_bits_again_and_from_any_row_block(eps, dev, f, heads):
    from eps_amd import ops
    c = gt.case(f, heads, "normal")
    d = _dev_case(c, dev)
    call = lambda lo, hi, **kw: ops.gat_aggregate(d["rowptr"][lo:hi + 1], d["col"], d["z"], d["s_src"], d["s_dst"], heads, row0=lo,
                                                  bias=d["bias"], want_lse=True, **kw)
    out, lse = call(0, gt.N_NODES)
    out2, lse2 = call(0, gt.N_NODES)
    assert _bits(out, out2) and _bits(lse, lse2)
    mid = gt.between_row(c["A"])
    for lo, hi in ((gt.LOOP_ROW, gt.LOOP_ROW + 1), (gt.LOOP_ONLY_ROW, gt.LOOP_ROW + 3), (gt.CHUNK_ROW, gt.CHUNK_ROW + 1),
                   (gt.CHUNK_ROW - 1, gt.HUB_ROW + 1), (mid, gt.N_NODES), (gt.N_NODES - 1, gt.N_NODES), (5, 5)):
        o, l = call(lo, hi)
        assert _bits(o, out[lo:hi]) and _bits(l, lse[lo:hi]), (lo, hi)
    # an empty row, and a row holding only its own stored self loop, give exactly z[i] + bias
    for i in (gt.EMPTY_ROW, gt.LOOP_ONLY_ROW):
        assert _bits(out[i], d["z"][i] + d["bias"])
    # a strided z (a column slice of a wider buffer) and a caller's strided out: the same bits
    wide = torch.full((gt.N_NODES, f + 8), float("nan"), device=dev)
    wide[:, 4:4 + f] = d["z"]
    buf = torch.full((gt.N_NODES, f + 4), float("nan"), device=dev)
    o = ops.gat_aggregate(d["rowptr"], d["col"], wide[:, 4:4 + f], d["s_src"], d["s_dst"], heads, bias=d["bias"], out=buf[:, :f])
    assert o.data_ptr() == buf.data_ptr() and _bits(buf[:, :f], out) and bool(torch.isnan(buf[:, f:]).all())
    # the two score tables as column blocks of one table
    s = torch.cat([d["s_src"], d["s_dst"], torch.full((gt.N_NODES, 3), float("nan"), device=dev)], 1)
    assert _bits(ops.gat_aggregate(d["rowptr"], d["col"], d["z"], s[:, :heads], s[:, heads:2 * heads], heads, bias=d["bias"]), out)


def test_operand_checks(eps, dev):
    from eps_amd import ops
    d = _dev_case(gt.case(8, 2, "normal"), dev)
    a = (d["rowptr"], d["col"])
    with pytest.raises(eps.EpsError, match="outside the kernel's domain"):
        ops.gat_aggregate(*a, d["z"], d["s_src"], d["s_dst"], 4)                               # C = 2
    with pytest.raises(eps.EpsError, match=r"s_src must be \[640, 2\]"):
        ops.gat_aggregate(*a, d["z"], d["s_src"][:, :1], d["s_dst"], 2)
    with pytest.raises(eps.EpsError, match="16-byte aligned rows"):
        ops.gat_aggregate(*a, torch.zeros((gt.N_NODES, 10), device=dev)[:, 1:9], d["s_src"], d["s_dst"], 2)
    with pytest.raises(eps.EpsError, match="bias holds 4 entries, not 8"):
        ops.gat_aggregate(*a, d["z"], d["s_src"], d["s_dst"], 2, bias=d["bias"][:4])
    with pytest.raises(eps.EpsError, match=r"rows \[600, 1240\) are outside"):
        ops.gat_aggregate(*a, d["z"], d["s_src"], d["s_dst"], 2, row0=600)
    with pytest.raises(eps.EpsError, match="rowptr holds 11 offsets"):
        ops.gat_aggregate_backward(d["rowptr"][:11], d["col"], d["z"], d["s_src"], d["s_dst"], 2, d["s_src"], d["z"], d["gout"])


# ----------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("f,heads", gt.SHAPES)
def test_backward_within_the_bounds(eps, dev, f, heads):
    """gz, g_s_src and g_s_dst in regime "quarters" (no raw score near the LeakyReLU kink) against the closed forms; the same
    bits on a second call; strided z and gout give the same bits as contiguous ones."""
    from eps_amd import ops
    c = gt.case(f, heads, "quarters")
    d = _dev_case(c, dev)
    a = (d["rowptr"], d["col"])
    out, lse = ops.gat_aggregate(*a, d["z"], d["s_src"], d["s_dst"], heads, want_lse=True)
    got = ops.gat_aggregate_backward(*a, d["z"], d["s_src"], d["s_dst"], heads, lse, out, d["gout"])
    tr = gt.aggregate_backward(c["rowptr"], c["col"], c["z"], c["s_src"], c["s_dst"], heads, out.cpu().numpy(), c["gout"])
    for name, g in zip(("gz", "g_s_src", "g_s_dst"), got):
        r = _ratio(name, g, tr[name], tr[name + "_bound"])
        scale = float(np.abs(tr[name]).max())
        print(f"\nf={f} heads={heads}: {name} largest error / bound {r:.3f} (largest bound / largest value {tr[name + '_bound'].max() / scale:.2e})")
        assert r <= 1.0 and bool(torch.isfinite(g).all())
        assert tr[name + "_bound"].max() <= 1e-2 * scale                   # a float32-sized bound (the hub row sums 301 terms), not a vacuous one
    again = ops.gat_aggregate_backward(*a, d["z"], d["s_src"], d["s_dst"], heads, lse, out, d["gout"])
    assert all(_bits(x, y) for x, y in zip(got, again))
    wz = torch.full((gt.N_NODES, f + 8), float("nan"), device=dev)
    wg = torch.full((gt.N_NODES, 2 * f + 4), float("nan"), device=dev)
    wz[:, 4:4 + f], wg[:, f:2 * f] = d["z"], d["gout"]
    strided = ops.gat_aggregate_backward(*a, wz[:, 4:4 + f], d["s_src"], d["s_dst"], heads, lse, out, wg[:, f:2 * f])
    assert all(_bits(x, y) for x, y in zip(got, strided))
    print(f"\nlargest device error / bound so far: {RATIOS}")


# ------------------------------------------------------------------------------------------------------------------ GATConv
def _exact_conv(eps, dev, heads=2, C=8, fin=8, seed=2):
    """A GATConv whose transform and scores are EXACT in float32 in any summation order (x in {-1, 0, 1}, lin.weight in
    {k/4}, att_* in {0, +-1/4, +-1/2}): train mode (torch products) and eval mode (ops.gemm) then hand the aggregate the same bits."""
    from eps_amd import models
    rng = np.random.default_rng(seed)
    conv = models.GATConv(fin, heads * C, heads).to(dev)
    with torch.no_grad():
        conv.lin.weight.copy_(torch.from_numpy(rng.integers(-2, 3, (heads * C, fin)) / 4.0))
        conv.att_src.copy_(torch.from_numpy(rng.integers(-2, 3, (1, heads, C)) / 4.0))
        conv.att_dst.copy_(torch.from_numpy(rng.integers(-2, 3, (1, heads, C)) / 4.0))
        conv.bias.copy_(torch.from_numpy(rng.standard_normal(heads * C)))
    x = torch.from_numpy(rng.integers(-1, 2, (gt.N_NODES, fin)).astype(np.float32)).to(dev)
    return conv, x


def _conv_truth(conv, x, A, relu):
    p = {k: v.detach().double().cpu().numpy() for k, v in conv.state_dict().items()}
    z = x.double().cpu().numpy() @ p["lin.weight"].T
    z3 = z.reshape(len(z), conv.heads, -1)
    s_src, s_dst = (z3 * p["att_src"]).sum(-1), (z3 * p["att_dst"]).sum(-1)
    assert np.array_equal(z, z.astype(np.float32)) and np.array_equal(s_src, s_src.astype(np.float32))      # exact in float32
    return gt.aggregate(A.indptr.astype(np.int64), A.indices, z, s_src, s_dst, conv.heads, p["bias"], relu, parts=True)


@pytest.mark.parametrize("relu", [False, True])
def test_conv_train_mode_equals_eval_mode(eps, dev, relu):
    A = gt.graph()
    adj = tgt._to_device_graph(eps, A, dev)
    conv, x = _exact_conv(eps, dev)
    tr = _conv_truth(conv, x, A, relu)
    conv.eval()
    ev = conv(x, adj, relu=relu)
    conv.train()
    trn = conv(x, adj, relu=relu)
    assert trn.requires_grad and not ev.requires_grad
    r_ev, r_tr = _ratio("conv eval", ev, tr["out"], tr["bound"]), _ratio("conv train", trn.detach(), tr["out"], tr["bound"])
    r_both = float(((trn.detach() - ev).abs().double().cpu().numpy() / tr["bound"]).max())
    print(f"\nGATConv relu={relu}: error / bound eval {r_ev:.3f}, train {r_tr:.3f}; |train - eval| / bound {r_both:.3f}")
    assert r_ev <= 1.0 and r_tr <= 1.0 and r_both <= 1.0
    # the row-block form gives the full layer's rows, bit for bit
    conv.eval()
    assert _bits(conv.forward_rows(x, adj, gt.LOOP_ROW, gt.LOOP_ROW + 70, relu=relu), ev[gt.LOOP_ROW:gt.LOOP_ROW + 70])


def test_conv_on_an_asymmetric_pattern(eps, dev):
    """Training needs the pattern to equal its transpose and says so; eval takes any graph and matches the truth."""
    B = gt.asymmetric(gt.graph())
    adj = tgt._to_device_graph(eps, B, dev)
    conv, x = _exact_conv(eps, dev, seed=3)
    conv.train()
    with pytest.raises(eps.EpsError, match="GATConv: training needs an adjacency with a symmetric pattern"):
        conv(x, adj)
    conv.eval()
    tr = _conv_truth(conv, x, B, False)
    assert _ratio("conv eval", conv(x, adj), tr["out"], tr["bound"]) <= 1.0
    with torch.no_grad():                                                  # no_grad in train mode scores too
        conv.train()
        assert _bits(conv(x, adj), conv.eval()(x, adj))


# ---------------------------------------------------------------------------------------------------------- model gradients
GRAD_SEED = 4        # chosen on the CPU: no raw attention score of the float64 forward lies within SCORE_MARGIN of zero (nearest: 1.98e-4)
ATT_SCALE = 8.0      # att_src / att_dst after their glorot draw, times this: scores a few units wide, so that attention is far from
                     # uniform and few of the 100 000 raw scores fall near zero (at the glorot scale no seed in 6000 keeps them all away)
SCORE_MARGIN = 1e-4


def test_model_gradients_match_float64(eps, dev):
    """LinkGNN with GAT (2 layers, H = 64, heads 4, dropout 0) and an H-wide embedding on a 1024-node R-MAT graph, 512 stored edges
    plus 512 random pairs: every parameter's gradient against float64 autograd through the dense formulation, by the project's
    own rule (tests/test_gpu_training.py, restated): |hip - f64| <= 2e-4 max(1e-6, max|f64|), and otherwise <= 4 times the
    distance of the float32 dense torch formulation from float64.  The gradients are compared on the branch of every ReLU the HIP
    forward took; LeakyReLU's kink is kept out of the way by the inputs themselves (asserted)."""
    from eps_amd import models
    adj = tgt._model_graph("unit", 10, dev, eps)
    n, H, heads = adj.n_rows, 64, 4
    assert n == 1024
    torch.manual_seed(GRAD_SEED)
    model = models.LinkGNN(torch.nn.Embedding(n, H), models.GAT(H, H, H, 2, 0.0, heads=heads), models.LinkPredictor(H, H, 1, 2, 0.0)).to(dev)
    with torch.no_grad():
        for conv in model.gnn.convs:
            conv.att_src.mul_(ATT_SCALE)
            conv.att_dst.mul_(ATT_SCALE)
    model.train()
    gen = torch.Generator().manual_seed(4)
    n_pos = 512
    edges = tgt._edge_batch(adj, n_pos, gen).to(dev)
    taken = []
    hooks = [m.register_forward_hook(lambda mod, inp, o: taken.append(o.detach() > 0))
             for m in list(model.gnn.convs[:-1]) + list(model.linkpred.lins[:-1])]
    out = model(None, edges, adj).squeeze(1)
    for h in hooks:
        h.remove()
    tt.log_loss(out, n_pos).backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values()) and len(taken) == 2 and len(grads) == 1 + 2 * 4 + 2 * 2
    mask = gt.dense_mask(adj.to_scipy(), dev)
    pre, raws = [], []
    with torch.no_grad():
        gt.link_gnn_forward(tt.params_as(model, torch.float64), mask, edges, heads, pre=pre, raws=raws)
    nearest = min(float(r[mask].abs().min()) for r in raws)
    print(f"\ngat gradients: the raw attention score nearest to zero in the float64 forward: {nearest:.3g}")
    assert len(raws) == 2 and nearest >= SCORE_MARGIN
    flips = 0
    for z, m in zip(pre, taken):
        differ = (z > 0) != m
        flips += int(differ.sum())
        assert float(z[differ].abs().max()) <= 1e-5 * max(1.0, float(z.abs().max())) if bool(differ.any()) else True
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = tt.params_as(model, dt)
        o = gt.link_gnn_forward(p, mask, edges, heads, branch=taken)
        tt.log_loss(o, n_pos).backward()
        ref[dt] = (o.detach(), {k: v.grad for k, v in p.items()})
    out_err = float((out.detach().double() - ref[torch.float64][0]).abs().max())
    print(f"\ngat: ReLU inputs whose sign differs between the HIP forward and float64: {flips}; train-mode scores, max |hip - f64| = "
          f"{out_err:.3g} (f32 dense: {float((ref[torch.float32][0].double() - ref[torch.float64][0]).abs().max()):.3g})")
    assert out_err < 1e-5
    tgt._check_grads("gat", grads, ref[torch.float64][1], ref[torch.float32][1], floor=1e-6)


# ------------------------------------------------------------------------------------------------------------ command lines
@pytest.fixture(scope="module")
def trained(eps, dev, tmp_path_factory):
    """rank.py --dataset ddi --model gat --synthetic on the 0.08 stand-in, once: the directory it ran in, its losses, its curve."""
    from eps_amd import rank_stage, training
    work = tmp_path_factory.mktemp("gat_cli")
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
        curves = rank_stage.main(["--dataset", "ddi", "--model", "gat", "--synthetic", "--hidden_channels", "32", "--epochs", "3",
                                  "--runs", "1", "--batch_size", "4096", "--save_models", "--eval_steps", "1"])
    finally:
        mp.undo()
    return dict(dir=work, losses=losses, curves=curves)


def test_rank_cli_trains_gat(trained):
    losses = trained["losses"]
    print(f"\nrank.py --model gat: losses {losses}")
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    curves = trained["curves"]
    assert len(curves) == 1 and 0.0 <= float(curves[0][1]) <= 100.0 and 0.0 <= float(curves[0][2]) <= 100.0
    assert [f for f in os.listdir(trained["dir"] / "models") if f.startswith("ddi_gat")] == ["ddi_gat||0|0.pt"]


def test_filter_cli_equals_the_restatement(eps, dev, trained, monkeypatch):
    """filter.py --model gat --keep_top K with the trained checkpoint == every candidate scored through model(x, pairs, adj) and
    ordered by the declared rule (proposals.sorted_edges_tensor: score descending, then the key order), exact on the pairs and on
    the scores; the row-sharded last layer under forward_sharded equals the full forward bit for bit."""
    monkeypatch.chdir(trained["dir"])
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.08")
    from eps_amd import candidates, datasets, filter_stage, graph, models, proposals
    argv = ["--dataset", "ddi", "--model", "gat", "--checkpoint", "ddi_gat||0|0.pt", "--synthetic", "--hidden_channels", "32"]
    args = models.default_model_configs(filter_stage.make_parser().parse_args(argv))
    ei, ew, _, data = datasets.get_data(args)
    data = data.to(dev)
    model = models.build_model(args, data, dev)
    assert type(model.gnn) is models.GAT and model.gnn.convs[0].heads == 4
    model.load_state_dict(torch.load("models/ddi_gat||0|0.pt", map_location=dev))
    model.eval()
    adj = graph.add_edges("ddi", ei.to(dev), ew.to(dev), torch.zeros((2, 0), dtype=torch.long, device=dev), data.num_nodes)
    with torch.no_grad():
        pairs = candidates.expand_block(adj, 0, adj.n_rows)[0]
        score = model(data.x, pairs, adj).reshape(-1)
        full = proposals.sorted_edges_tensor(pairs, score).cpu()
    assert full.shape[0] > 5000 and len(torch.unique(full[:, 2])) > 1000
    got = torch.load(filter_stage.main(argv + ["--keep_top", "1000"]))
    assert got.shape == (1000, 3) and got.dtype == torch.float32 and torch.equal(got, full[:1000])
    # the row-sharded last layer (virtual ranks 0..3 on one GPU), as test_row_sharded_last_layer_equals_full_forward emulates it
    xin = model._node_input(data.x)
    whole = model.gnn(xin, adj)
    parts = [model.gnn.forward_sharded(xin, adj, rank, 4, lambda local, bounds: local) for rank in range(4)]
    assert torch.equal(torch.cat(parts, 0), whole) and _bits(whole, model.embeddings(data.x, adj))


def test_gat_takes_the_routes_of_a_link_gnn(eps, dev, trained, monkeypatch):
    """What a LinkGNN with a LinkPredictor takes, gat takes: training through the fused decode (rank.py --fused_decode) and the
    bf16 screening decode of the filter, whose rows carry the fp32 score of their pair bit for bit."""
    monkeypatch.chdir(trained["dir"])
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.08")
    from eps_amd import filter_stage, rank_stage, training
    losses = []
    orig = training.train
    monkeypatch.setattr(rank_stage, "train", lambda *a, **k: losses.append(orig(*a, **k)) or losses[-1])
    torch.manual_seed(1)
    rank_stage.main(["--dataset", "ddi", "--model", "gat", "--synthetic", "--hidden_channels", "32", "--gat_heads", "2", "--epochs", "2",
                     "--runs", "1", "--batch_size", "4096", "--eval_steps", "2", "--fused_decode"])
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    argv = ["--dataset", "ddi", "--model", "gat", "--checkpoint", "ddi_gat||0|0.pt", "--synthetic", "--hidden_channels", "32"]
    whole = torch.load(filter_stage.main(argv))
    fp32 = {(int(u), int(v)): float(sc) for u, v, sc in whole.tolist()}
    got = torch.load(filter_stage.main(argv + ["--keep_top", "1000", "--decode_precision", "bf16"]))
    assert got.shape == (1000, 3) and bool((got[:-1, 2] >= got[1:, 2]).all())
    assert all(fp32[(int(u), int(v))] == float(sc) for u, v, sc in got.tolist())
