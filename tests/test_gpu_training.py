"""GPU: the training path (train_and_eval.py:31-96 restated): gradients of the HIP-SpMM autograd Function vs a dense
torch formulation, a short rank.py run that trains a GCN rank model and saves a checkpoint filter.py can load, and -- against
the float64 truth of tests/training_truth.py -- models._SpMM itself at the kernel's staging boundaries, the convs' guards,
model gradients at dataset-like widths and a few optimiser steps."""
import argparse
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import training_truth as tt
from layer_truth import rows_graph as _rows_graph, symmetric_weights as _symmetric_weights

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_gradients_match_dense_formulation(eps, dev, kind):
    from eps_amd import models, synth
    torch.manual_seed(0)
    g = synth.rmat_graph(8, 6, 4, "cpu")
    n = g.n_rows
    A = torch.from_numpy(g.to_scipy().toarray()).float().to(dev)
    adj = g.to(dev)
    H, fin = 16, 12
    cls = models.GCN if kind == "gcn" else models.SAGE
    model = models.LinkGNN(torch.nn.Embedding(n, H), cls(fin + H, H, H, 2, 0.0), models.LinkPredictor(H, H, 1, 2, 0.0)).to(dev)
    model.train()
    x = torch.randn(n, fin, device=dev)
    edges = torch.randint(0, n, (2, 300), device=dev)
    out = model(x, edges, adj).squeeze()
    loss = -torch.log(out[:150] + 1e-8).mean() - torch.log(1 - out[150:] + 1e-8).mean()
    loss.backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}

    # dense reference of the same forward on torch autograd
    for p in model.parameters():
        p.grad = None
    xin = torch.cat([model.emb.weight, x], 1)
    if kind == "gcn":
        Ah = A.clone(); Ah.fill_diagonal_(1.0)
        dis = Ah.sum(1).pow(-0.5)
        An = dis[:, None] * Ah * dis[None, :]
        h = xin
        for i, conv in enumerate(model.gnn.convs):
            h = An @ (h @ conv.weight) + conv.bias
            if i == 0:
                h = torch.relu(h)
    else:
        M = (A != 0).float()
        Dn = M / M.sum(1).clamp(min=1)[:, None]
        h = xin
        for i, conv in enumerate(model.gnn.convs):
            h = conv.lin_l(Dn @ h) + conv.lin_r(h)
            if i == 0:
                h = torch.relu(h)
    z = h[edges[0]] * h[edges[1]]
    z = torch.relu(model.linkpred.lins[0](z))
    ref = torch.sigmoid(model.linkpred.lins[1](z)).squeeze()
    assert float((ref.detach() - out.detach()).abs().max()) < 1e-5
    loss_ref = -torch.log(ref[:150] + 1e-8).mean() - torch.log(1 - ref[150:] + 1e-8).mean()
    loss_ref.backward()
    for k, p in model.named_parameters():
        scale = max(1e-6, float(p.grad.abs().max()))
        assert float((p.grad - grads[k]).abs().max()) <= 2e-4 * scale, k


def test_rank_cli_trains_and_filter_loads_checkpoint(eps, tmp_path, monkeypatch):
    """rank.py --model gcn on the ddi stand-in: loss goes down, Hits are produced, the best-valid checkpoint is written
    under the reference's name pattern and filter.py scores candidates with it."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.08")
    from eps_amd import filter_stage, rank_stage, training
    losses = []
    orig = training.train

    def spy(*a, **k):
        losses.append(orig(*a, **k))
        return losses[-1]

    monkeypatch.setattr(rank_stage, "train", spy)
    torch.manual_seed(1)
    curves = rank_stage.main(["--dataset", "ddi", "--model", "gcn", "--runs", "1", "--epochs", "12", "--synthetic",
                              "--hidden_channels", "32", "--batch_size", "4096", "--save_models", "--eval_steps", "4"])
    assert len(losses) == 12 and min(losses[-3:]) < losses[0] - 0.02, losses    # BCE starts at 2 ln 2 = 1.386
    assert len(curves) == 1 and 0.0 <= float(curves[0][1]) <= 100.0
    ckpts = [f for f in os.listdir("models") if f.startswith("ddi_gcn||0|0")]
    assert ckpts == ["ddi_gcn||0|0.pt"]
    fname = filter_stage.main(["--dataset", "ddi", "--model", "gcn", "--checkpoint", "ddi_gcn||0|0.pt", "--synthetic",
                               "--hidden_channels", "32", "--keep_top", "1000"])
    got = torch.load(fname)
    assert got.shape == (1000, 3) and bool((got[:-1, 2] >= got[1:, 2]).all()) and 0.0 < float(got[0, 2]) <= 1.0


# ====================================================================================================================
# The training path against the float64 truth of tests/training_truth.py (validated on the CPU by test_training_host.py)
# ====================================================================================================================
U = 2.0 ** -24                                   # unit roundoff of float32: every correctly rounded operation errs by <= U relative

BOUNDARY_ROWS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2049, 4200]     # SP_FLIGHT = 32 rows, fetches of 64 entries, one hub
WIDTHS = [1, 3, 58, 64, 256, 260, 314, 384]      # scalar kernel (1, 3, 58, 314), float4 kernel, and a second column pass (> 256)


def _spmm_graph(kind):
    """float64 scipy CSR, symmetric in pattern and values."""
    from eps_amd import synth
    rng = np.random.default_rng(17)
    if kind == "rows":
        return _rows_graph(rng, BOUNDARY_ROWS, 4500)
    A = synth.rmat_graph(10, 8, 5, "cpu").to_scipy().astype(np.float64)
    n = A.shape[0]
    if kind == "unit":
        return A
    if kind == "weighted":                       # collab: values are sums over duplicate edges
        m = 6000                                                      # half of the edges inside a 32 x 256 block: many duplicates
        r = np.concatenate([rng.integers(0, 32, m), rng.integers(0, n, m)])
        c = np.concatenate([rng.integers(0, 256, m), rng.integers(0, n, m)])
        keep = r != c
        W = ssp.coo_matrix((np.ones(keep.sum()), (r[keep], c[keep])), shape=(n, n)).tocsr()   # duplicates summed ...
        W = (W + W.T).tocsr()                                                                 # ... and again by to_symmetric
        assert W.data.max() >= 4
        return W
    if kind == "loops":                          # stored self loops with values other than 1 on a third of the nodes
        d = np.zeros(n)
        d[::3] = rng.integers(2, 5, len(d[::3]))
        return (_symmetric_weights(A, rng) + ssp.diags(d)).tocsr()
    if kind == "isolated":                       # several isolated rows: scattered ones and a block at the end
        gone = np.zeros(n, bool)
        gone[rng.choice(n, 40, replace=False)] = True
        gone[-25:] = True
        keep = ssp.diags((~gone).astype(np.float64))
        B = (keep @ A @ keep).tocsr()
        B.eliminate_zeros()
        assert (np.diff(B.indptr) == 0).sum() >= 65
        return B
    raise ValueError(kind)


def _to_device_graph(eps, A, dev):
    A = ssp.csr_matrix(A, dtype=np.float32)
    A.sort_indices()
    return eps.CSRGraph.from_scipy(A, device=dev)


# Extra roundings of the BACKWARD next to the deg_row roundings of the product's own fma chain, in units of U:
#   sum on the adjacency itself: none -- the stored matrix equals its transpose bit for bit, dX = A dY is the closed form.
#   gcn / tag normalised copy:   4 -- the closed form multiplies by B^T, the kernel by B, B = fl(fl(val * dis[r]) * dis[c]); an
#                                entry and its mirror are each two roundings away from the same exact product, so they differ
#                                by at most 4 U relative (the "one rounding" asymmetry; typically one ulp).
#   mean:                        2 -- inv = fl(1 / deg) and fl(dY * inv) before the product (the forward's division comes AFTER
#                                its deg - 1 additions and is counted in deg).
# The forward has no extra rounding in any mode.  The bound is the standard gamma_k = k U / (1 - k U), k = deg_row + c, times
# the product of absolute values.
C_BWD = {"sum": 0, "gcn": 4, "tag": 4, "mean": 2}


def _gamma(k):
    return k * U / (1.0 - k * U)


def _ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; an element whose bound is 0 (an empty row) must be exact."""
    err = np.abs(got.astype(np.float64) - ref)
    zero = bound == 0
    assert float(err[zero].max(initial=0.0)) == 0.0
    return float((err[~zero] / bound[~zero]).max(initial=0.0))


def _matrices(adj):
    return [("sum", adj, False), ("gcn", adj.gcn_normalized(), False), ("tag", adj.tag_normalized(), False), ("mean", adj, True)]


@pytest.mark.parametrize("kind", ["unit", "weighted", "loops", "isolated", "rows"])
def test_spmm_function_vs_float64(eps, dev, kind):
    """models._SpMM forward and backward against the scipy float64 closed forms (Y = B X, dX = B^T dY; mean: D^-1 P), B the
    float32 matrix the kernel multiplies by.  Per element |err| <= gamma(deg_row + c) * (|B| |X|), c counted above."""
    from eps_amd import models
    adj = _to_device_graph(eps, _spmm_graph(kind), dev)
    n = adj.n_rows
    rng = np.random.default_rng(23)
    worst = {}
    for name, g, mean in _matrices(adj):
        B = g.to_scipy().astype(np.float64)
        Babs = abs(B)
        deg = np.diff(B.indptr).astype(np.float64)[:, None]
        if kind == "rows" and name != "gcn":
            assert deg[:len(BOUNDARY_ROWS), 0].tolist() == BOUNDARY_ROWS
        for f in WIDTHS:
            x = rng.standard_normal((n, f)).astype(np.float32)
            gy = rng.standard_normal((n, f)).astype(np.float32)
            xd = torch.from_numpy(x).to(dev).requires_grad_(True)
            y = models._SpMM.apply(xd, g, mean)
            y.backward(torch.from_numpy(gy).to(dev))
            r_f = _ratio(y.detach().cpu().numpy(), tt.spmm_forward(B, x, mean), _gamma(deg) * tt.spmm_forward(Babs, np.abs(x), mean))
            r_b = _ratio(xd.grad.cpu().numpy(), tt.spmm_backward(B, gy, mean),
                         _gamma(deg + C_BWD[name]) * tt.spmm_backward(Babs, np.abs(gy), mean))
            worst[(name, "fwd")] = max(worst.get((name, "fwd"), 0.0), r_f)
            worst[(name, "bwd")] = max(worst.get((name, "bwd"), 0.0), r_b)
            assert r_f <= 1.0 and r_b <= 1.0, (kind, name, f, r_f, r_b)
    print(f"\n_SpMM vs float64 [{kind}] largest error / bound: " + ", ".join(f"{k[0]}.{k[1]} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("f", [58, 256, 314])
def test_spmm_function_strided_inputs_and_determinism(eps, dev, f):
    """x as a column slice of a wider tensor, grad_out non-contiguous (a transposed buffer; the gradient of a column slice of
    the output), and two backward runs bit-identical (the kernel accumulates sequentially, in stored order)."""
    from eps_amd import models
    adj = _to_device_graph(eps, _spmm_graph("loops"), dev)
    n = adj.n_rows
    rng = np.random.default_rng(29)
    for name, g, mean in _matrices(adj):
        B = g.to_scipy().astype(np.float64)
        deg = np.diff(B.indptr).astype(np.float64)[:, None]
        wide = torch.from_numpy(rng.standard_normal((n, f + 9)).astype(np.float32)).to(dev).requires_grad_(True)
        x = wide[:, 5:5 + f]
        assert not x.is_contiguous()
        gy = torch.from_numpy(rng.standard_normal((f, n)).astype(np.float32)).to(dev).t()      # [n, f], strides (1, n)
        assert not gy.is_contiguous()
        seen = []
        y = models._SpMM.apply(x, g, mean)
        y.register_hook(lambda t: seen.append(t.is_contiguous()))
        y.backward(gy)
        assert seen == [False]
        x_np, gy_np = x.detach().cpu().numpy(), gy.cpu().numpy()
        assert _ratio(y.detach().cpu().numpy(), tt.spmm_forward(B, x_np, mean),
                      _gamma(deg) * tt.spmm_forward(abs(B), np.abs(x_np), mean)) <= 1.0, name
        got = wide.grad.cpu().numpy()
        assert not got[:, :5].any() and not got[:, 5 + f:].any()
        assert _ratio(got[:, 5:5 + f], tt.spmm_backward(B, gy_np, mean),
                      _gamma(deg + C_BWD[name]) * tt.spmm_backward(abs(B), np.abs(gy_np), mean)) <= 1.0, name
        first = wide.grad.clone()
        wide.grad = None
        models._SpMM.apply(x, g, mean).backward(gy)
        assert torch.equal(wide.grad, first), name
        # the gradient of a column slice of the output: zero outside the slice
        wide.grad = None
        lo, hi = 1, max(2, f - 3)
        w = torch.from_numpy(rng.standard_normal((n, hi - lo)).astype(np.float32)).to(dev)
        (models._SpMM.apply(x, g, mean)[:, lo:hi] * w).sum().backward()
        gs = np.zeros((n, f), np.float32)
        gs[:, lo:hi] = w.cpu().numpy()
        assert _ratio(wide.grad.cpu().numpy()[:, 5:5 + f], tt.spmm_backward(B, gs, mean),
                      _gamma(deg + C_BWD[name]) * tt.spmm_backward(abs(B), np.abs(gs), mean)) <= 1.0, name


# ---------------------------------------------------------------------------------------------------------- guards
class _Launched(Exception):
    pass


def _asymmetric_values_graph(eps, dev):
    """Symmetric pattern, values 4x larger above the diagonal than below it."""
    A = _spmm_graph("weighted")
    B = (A + 3.0 * ssp.triu(A, 1)).tocsr()
    assert (B != B.T).nnz > 100 and (tt.pattern_of(B) != tt.pattern_of(B).T).nnz == 0
    return _to_device_graph(eps, B, dev), B


def _convs(fin, dev):
    from eps_amd import models
    torch.manual_seed(5)
    return {"gcn": models.GCNConv(fin, 8).to(dev), "sage": models.SAGEConv(fin, 8).to(dev), "tag": models.TAGConv(fin, 8, 2).to(dev)}


def test_convs_refuse_what_the_backward_cannot_take(eps, dev, monkeypatch):
    """Training mode: a directed pattern is refused by GCNConv, SAGEConv and TAGConv, asymmetric values on a symmetric pattern
    by GCNConv and TAGConv (SAGEConv's mean does not read them), a row-count mismatch by all three in both modes -- each before
    the SpMM or the normalisation kernel is launched.  The same graphs score under eval()."""
    from eps_amd import ops
    from test_gpu_cosine_cn import directed_graph
    Ad = directed_graph(200, 1500, seed=1)
    directed = _to_device_graph(eps, Ad, dev)
    skewed, As = _asymmetric_values_graph(eps, dev)
    fin = 12
    convs = _convs(fin, dev)

    def boom(*a, **k):
        raise _Launched()

    with monkeypatch.context() as mp:
        mp.setattr(ops, "spmm_csr", boom)
        mp.setattr(ops, "gcn_norm", boom)
        for g in (directed, skewed):
            x = torch.randn(g.n_rows, fin, device=dev, requires_grad=True)
            for name, conv in convs.items():
                conv.train()
                if g is skewed and name == "sage":
                    with pytest.raises(_Launched):           # accepted: it gets as far as the (disabled) kernel
                        conv(x, g)
                    continue
                with pytest.raises(eps.EpsError, match="symmetric"):
                    conv(x, g)
            for mode in ("train", "eval"):
                short = torch.randn(g.n_rows - 1, fin, device=dev)
                for name, conv in convs.items():
                    getattr(conv, mode)()
                    with pytest.raises(ValueError, match="one row per column"):
                        conv(short, g)
        x = torch.randn(directed.n_rows - 1, fin, device=dev)
        with pytest.raises(ValueError, match="one row per column"):
            convs["tag"].hops(x, directed)
        for name in ("gcn", "sage"):
            with pytest.raises(ValueError, match="one row per column"):
                convs[name].forward_rows(x, directed, 0, 10)

    # eval / no_grad: no symmetry needed -- the forward on these graphs matches the float64 restatement
    for g, A in ((directed, Ad), (skewed, As)):
        x = torch.randn(g.n_rows, fin, device=dev)
        A64 = torch.from_numpy(ssp.csr_matrix(A).toarray()).double().to(dev)
        P64 = torch.from_numpy(tt.pattern_of(A).toarray()).double().to(dev)
        x64 = x.double()
        refs = {"gcn": tt.gcn_matrix(A64) @ (x64 @ convs["gcn"].weight.double()) + convs["gcn"].bias.double(),
                "sage": (tt.mean_matrix(P64) @ x64) @ convs["sage"].lin_l.weight.double().t() + convs["sage"].lin_l.bias.double()
                        + x64 @ convs["sage"].lin_r.weight.double().t()}
        An = tt.tag_matrix(A64)
        refs["tag"] = (torch.cat([x64, An @ x64, An @ (An @ x64)], 1) @ convs["tag"].lin.weight.double().t()
                       + convs["tag"].lin.bias.double())
        for name, conv in convs.items():
            outs = [conv.eval()(x, g)]
            conv.train()
            with torch.no_grad():
                outs.append(conv(x, g))
            for out in outs:
                ref = refs[name].detach()
                assert float((out.detach().double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), name
    # ... and SAGEConv trains on the asymmetric VALUES: its gradient in x is the pattern's closed form
    conv = convs["sage"].train()
    x = torch.randn(skewed.n_rows, fin, device=dev, requires_grad=True)
    conv(x, skewed).sum().backward()
    ones = np.ones((skewed.n_rows, 8))
    ref = tt.spmm_backward(As, ones @ conv.lin_l.weight.detach().double().cpu().numpy(), True) \
        + ones @ conv.lin_r.weight.detach().double().cpu().numpy()
    assert float(np.abs(x.grad.cpu().numpy() - ref).max()) <= 2e-5 * max(1.0, float(np.abs(ref).max()))


# ---------------------------------------------------------------------------------------------------------- model gradients
GATE = 2e-4          # the project's gradient gate (test_gradients_match_dense_formulation, test_gpu_dea): per parameter, of max|grad|


def _model_graph(kind, scale, dev, eps):
    """R-MAT graph of 2**scale nodes: 'unit', or 'weighted' = symmetric integer weights and stored self loops (collab-like)."""
    from eps_amd import synth
    A = synth.rmat_graph(scale, 8, 7, "cpu").to_scipy().astype(np.float64)
    if kind == "weighted":
        rng = np.random.default_rng(31)
        d = np.zeros(A.shape[0])
        d[::4] = rng.integers(1, 4, len(d[::4]))
        A = (_symmetric_weights(A, rng) + ssp.diags(d)).tocsr()
    return _to_device_graph(eps, A, dev)


def _edge_batch(adj, n_pos, gen):
    """[2, 2 n_pos] int64 on the CPU: n_pos stored edges of the graph, then n_pos uniformly drawn pairs."""
    row, col, _ = adj.cpu().coo()
    pick = torch.randint(0, row.numel(), (n_pos,), generator=gen)
    neg = torch.randint(0, adj.n_rows, (2, n_pos), generator=gen)
    return torch.cat([torch.stack([row[pick], col[pick]]), neg], 1)


def _check_grads(tag, named_grads, g64, g32, floor):
    """Per parameter: |hip - f64| <= GATE * max(floor, max|f64|); a parameter past that gate is held to 4x the distance of the
    float32 dense torch formulation from float64 instead (the summation orders differ -- sequential per row against blocked
    BLAS -- which changes the rounding, not the operation).  -> the largest ratios, for the log."""
    worst_gate, worst_f32, fell_back = 0.0, 0.0, []
    for k, g in named_grads.items():
        err = float((g.double() - g64[k]).abs().max())
        d32 = float((g32[k].double() - g64[k]).abs().max())
        gate = GATE * max(floor, float(g64[k].abs().max()))
        worst_gate = max(worst_gate, err / gate)
        if d32 > 0:
            worst_f32 = max(worst_f32, err / d32)
        if err > gate:
            fell_back.append((k, err / gate, err / max(d32, 1e-300)))
            assert err <= 4.0 * d32, (tag, k, err, gate, d32)
    print(f"\n{tag}: largest |hip - f64| / gate {worst_gate:.3f}; largest |hip - f64| / |f32 dense - f64| {worst_f32:.2f}; "
          f"past the {GATE:g} gate (held to 4x f32 dense): {fell_back}")
    return worst_gate, worst_f32


@pytest.mark.parametrize("kind", ["gcn", "sage"])
@pytest.mark.parametrize("shape", ["ppa", "collab", "ddi"])
def test_model_gradients_at_dataset_shapes(eps, dev, kind, shape):
    """LinkGNN (3 layers, H = 256, dropout 0) on a 2048-node R-MAT graph: every parameter's gradient, emb.weight included, and
    the train-mode scores against the float64 restatement.  ppa-like: unit graph, 58 features + 256 embedding = 314 columns
    (the scalar SpMM kernel); collab-like: weighted graph with self loops, 128 + 256; ddi-like: the embedding alone."""
    from eps_amd import models
    graph_kind, fin = {"ppa": ("unit", 58), "collab": ("weighted", 128), "ddi": ("unit", 0)}[shape]
    adj = _model_graph(graph_kind, 11, dev, eps)
    n, H = adj.n_rows, 256
    assert n <= 2048
    torch.manual_seed(3)
    cls = models.GCN if kind == "gcn" else models.SAGE
    model = models.LinkGNN(torch.nn.Embedding(n, H), cls(fin + H, H, H, 3, 0.0), models.LinkPredictor(H, H, 1, 3, 0.0)).to(dev)
    model.train()
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, fin, generator=gen).to(dev) if fin else None
    n_pos = 2048
    edges = _edge_batch(adj, n_pos, gen).to(dev)
    taken = []                                   # the branch of every ReLU the HIP forward took, in forward order
    hooks = [m.register_forward_hook(lambda mod, inp, o: taken.append(o.detach() > 0))
             for m in list(model.gnn.convs[:-1]) + list(model.linkpred.lins[:-1])]
    out = model(x, edges, adj).squeeze(1)
    for h in hooks:
        h.remove()
    tt.log_loss(out, n_pos).backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values()) and len(taken) == 4
    # ReLU has no derivative at 0.  Where the float32 forward and the float64 one take different branches, the float64
    # pre-activation must be one float32 cannot tell from 0 (within the forward gate, 1e-5 of the layer's scale); the gradients
    # are then compared on the branch the HIP forward took, for the float64 truth and the float32 dense formulation alike.
    pre = []
    with torch.no_grad():
        tt.link_gnn_forward(kind, tt.params_as(model, torch.float64), tt.dense_adjacency(adj, torch.float64, dev),
                            tt.dense_pattern(adj, torch.float64, dev), x, edges, pre=pre)
    flips = 0
    for z, mask in zip(pre, taken):
        differ = (z > 0) != mask
        flips += int(differ.sum())
        assert float(z[differ].abs().max()) <= 1e-5 * max(1.0, float(z.abs().max())) if bool(differ.any()) else True
    print(f"\n{kind}/{shape}: ReLU inputs whose sign differs between the HIP forward and float64: {flips}")
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = tt.params_as(model, dt)
        A, P = tt.dense_adjacency(adj, dt, dev), tt.dense_pattern(adj, dt, dev)
        o = tt.link_gnn_forward(kind, p, A, P, x, edges, branch=taken)
        tt.log_loss(o, n_pos).backward()
        ref[dt] = (o.detach(), {k: v.grad for k, v in p.items()})
    out_err = float((out.detach().double() - ref[torch.float64][0]).abs().max())
    print(f"\n{kind}/{shape}: train-mode scores, max |hip - f64| = {out_err:.3g} "
          f"(f32 dense: {float((ref[torch.float32][0].double() - ref[torch.float64][0]).abs().max()):.3g})")
    assert out_err < 1e-5
    _check_grads(f"{kind}/{shape}", grads, ref[torch.float64][1], ref[torch.float32][1], floor=1e-6)


# ---------------------------------------------------------------------------------------------------------- optimiser steps
def _sgd_steps(params, loss_of, batches, lr):
    """Plain SGD with training.train's clipping; -> (loss on the first batch before the first step, the same after the last)."""
    params = list(params)
    opt = torch.optim.SGD(params, lr=lr)
    first = None
    for b in batches:
        opt.zero_grad()
        loss = loss_of(b)
        first = float(loss.detach()) if first is None else first
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    return first, float(loss_of(batches[0]).detach())


@pytest.mark.parametrize("kind", ["gcn", "sage", "dea"])
def test_optimiser_steps_follow_float64_replica(eps, dev, kind):
    """Five optimiser steps on fixed edge batches of one weighted graph (dropout 0, clip_grad_norm_ at 1.0 like training.train):
    the HIP path, a float32 dense torch replica and a float64 dense torch replica start from the same parameters and see the
    same batches.  Per parameter, the HIP path ends no further from the float64 replica than 4x the float32 dense replica's
    own distance, plus one float32 ulp of the parameter's magnitude; the loss on the first batch falls in all three.

    Plain SGD, not the Adam of rank.py: Adam divides the step by sqrt(v), which turns float32 NOISE into a full +-lr step on
    every parameter whose true gradient is 0 (DEA's biases in front of a training-mode BatchNorm are such parameters), so an
    Adam trajectory measures the sign of rounding errors, not precision."""
    from eps_amd import models
    adj = _model_graph("weighted", 10, dev, eps)
    n, H, fin, n_pos, lr = adj.n_rows, 64, 20, 512, 0.5
    torch.manual_seed(6)
    if kind == "dea":
        model = models.DEA_GNN_JK(n, H, H + fin, H, H, 3, H, H, 1, 2, 0.0, True, True, 2, "max").to(dev)
    else:
        cls = models.GCN if kind == "gcn" else models.SAGE
        model = models.LinkGNN(torch.nn.Embedding(n, H), cls(fin + H, H, H, 3, 0.0), models.LinkPredictor(H, H, 1, 3, 0.0)).to(dev)
    model.train()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(n, fin, generator=gen).to(dev)
    batches = [_edge_batch(adj, n_pos, gen).to(dev) for _ in range(5)]
    label = torch.cat([torch.ones(n_pos), torch.zeros(n_pos)]).to(dev)

    replicas = {}
    for dt in (torch.float64, torch.float32):                      # copies of the INITIAL parameters: made before any step
        replicas[dt] = tt.params_as(model, dt, buffers=True)
    losses, final = {}, {}
    for dt, p in replicas.items():
        A, P = tt.dense_adjacency(adj, dt, dev), tt.dense_pattern(adj, dt, dev)
        if kind == "dea":
            loss_of = lambda b: tt.bce_logits_loss(tt.dea_forward(p, A, x, b, "max"), label)
        else:
            loss_of = lambda b: tt.log_loss(tt.link_gnn_forward(kind, p, A, P, x, b), n_pos)
        losses[dt] = _sgd_steps([v for v in p.values() if v.requires_grad], loss_of, batches, lr)
        final[dt] = {k: v.detach().double() for k, v in p.items() if v.requires_grad}
    if kind == "dea":
        hip_loss = lambda b: model.loss(model(x, b, adj), label)
    else:
        hip_loss = lambda b: tt.log_loss(model(x, b, adj).squeeze(1), n_pos)
    losses["hip"] = _sgd_steps(model.parameters(), hip_loss, batches, lr)
    for who, (first, last) in losses.items():
        assert last < first, (who, first, last)
    worst = 0.0
    for k, p in model.named_parameters():
        p64 = final[torch.float64][k]
        d_hip = float((p.detach().double() - p64).abs().max())
        d_f32 = float((final[torch.float32][k] - p64).abs().max())
        ulp = 2.0 ** -23 * float(p64.abs().max())
        worst = max(worst, d_hip / (4.0 * d_f32 + ulp))
        assert d_hip <= 4.0 * d_f32 + ulp, (k, d_hip, d_f32, ulp)
    print(f"\n{kind}: 5 SGD steps, losses (first batch: before, after) {losses}; largest |hip - f64| / (4 |f32 dense - f64| + ulp) "
          f"= {worst:.3f}")
