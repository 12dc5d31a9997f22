"""GPU: dea's fused training decode with BatchNorm on batch statistics (csrc/mlp_decode_train.hip: ops.mlp_decode_bn_stats, the
folded ops.mlp_decode_train, ops.mlp_decode_bn_backward; DEA_GNN_JK.fused_decode; rank.py --fused_decode_bn) against the float64
restatement of tests/decode_bn_cases.py and tests/training_truth.py.  N = 50 nodes, so endpoints collide; every batch holds a
self pair and (from three edges on) a duplicated pair; B crosses the 64-edge tile, H = 32 is the minimum, 36 takes the pad columns,
256 is the full tile."""
import os

import numpy as np
import pytest
import torch

import decode_bn_cases as bc
import decode_train_cases as dc
import training_truth as tt

pytestmark = pytest.mark.gpu

EPS = tt.BN_EPS


def _to_dev(case, dev):
    h, edges, ws, bs, gamma, beta, keep = case
    return dict(h=h.to(dev), u=edges[0].to(dev, torch.int32), v=edges[1].to(dev, torch.int32), ws=[w.to(dev) for w in ws],
                bs=[b.to(dev) for b in bs], gamma=gamma.to(dev), beta=beta.to(dev))


def _hip_step(eps, d, keep_words, scale):
    """Statistics, folded forward (with its taken bits), BCE on the logits, backward -> (mean, var, logits, taken, grads)."""
    from eps_amd import models
    ops = eps.ops
    mean, var = ops.mlp_decode_bn_stats(d["h"], d["u"], d["v"], d["ws"], d["bs"])
    wf, bf = models.fold_batch_statistics(d["ws"][0], d["bs"][0], d["gamma"], d["beta"], mean, var, EPS)
    out, taken = ops.mlp_decode_train(d["h"], d["u"], d["v"], [wf, d["ws"][1]], [bf, d["bs"][1]], keep=keep_words, keep_scale=scale,
                                      apply_sigmoid=False, want_taken=True)
    leaf = out.clone().requires_grad_(True)
    tt.bce_logits_loss(leaf, bc.labels(out.numel()).to(out.device)).backward()
    gh, gw, gb, gg, gbeta = ops.mlp_decode_bn_backward(d["h"], d["u"], d["v"], d["ws"], d["bs"], wf, bf, d["gamma"], mean, var, EPS,
                                                       leaf.grad.contiguous(), keep=keep_words, keep_scale=scale)
    grads = {"h": gh, "w0": gw[0], "w1": gw[1], "b0": gb[0], "b1": gb[1], "gamma": gg, "beta": gbeta}
    return mean, var, out, taken, grads


def _check_case(eps, dev, tag, case, masked):
    h, edges, ws, bs, gamma, beta, keep = case
    H = h.shape[1]
    d = _to_dev(case, dev)
    kp, scale = (keep, 2.0) if masked else (None, 1.0)
    kw = eps.ops.pack_mask(keep.to(dev)).unsqueeze(0).contiguous() if masked else None
    mean, var, out, taken, got = _hip_step(eps, d, kw, scale)
    f64 = lambda xs: [x.double() for x in xs]   # noqa: E731
    m64, v64 = bc.statistics(h.double(), edges, f64(ws), f64(bs))
    for name, g, r in (("mean", mean, m64), ("var", var, v64)):
        err = (g.double().cpu() - r).abs()
        print(f"\n{tag} {name}: max |hip - f64| = {float(err.max()):.3g}")
        assert bool((err <= 1e-5 * r.abs().clamp(min=1.0)).all()), name
    ref = bc.bn_forward(h.double(), edges, f64(ws), f64(bs), gamma.double(), beta.double(), kp, scale)
    err = float((out.double().cpu() - ref).abs().max())
    print(f"{tag} logits: max |hip - f64| = {err:.3g}")
    assert torch.isfinite(out).all() and err <= 1e-4 * max(1.0, float(ref.abs().max()))
    branch = eps.ops.unpack_mask(taken, H)[0].cpu()
    g64 = bc.reference_grads(h, edges, ws, bs, gamma, beta, kp, scale, branch, torch.float64)
    g32 = bc.reference_grads(h, edges, ws, bs, gamma, beta, kp, scale, branch, torch.float32)
    assert set(got) == set(g64) and all(tuple(got[k].shape) == tuple(g64[k].shape) for k in got)
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    dc.check_grads(tag, got, g64, g32)
    assert int(torch.count_nonzero(got["b0"])) == 0        # exact zeros, not float noise
    return v64


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,B", bc.SHAPES)
def test_statistics_logits_and_gradients_match_float64(eps, dev, H, B, masked):
    _check_case(eps, dev, f"H={H} B={B} masks={masked}", bc.make_case(H, B, bc.seed_of(H, B)), masked)


@pytest.mark.parametrize("masked", [False, True])
def test_channel_of_zero_variance(eps, dev, masked):
    """A zero row of W0: that channel's pre-activation is b0 on every edge, its variance 0 and sigma = sqrt(eps)."""
    case = bc.make_case(64, 65, 4242, zero_row=5)
    v64 = _check_case(eps, dev, f"zero variance masks={masked}", case, masked)
    assert float(v64[5]) == 0.0


@pytest.mark.parametrize("masked", [False, True])
def test_shifted_mean(eps, dev, masked):
    """h = 1 + 0.02 * randn: the products sit at 1 with a spread of 0.03, so a channel's mean is the row sum of W0 while its
    spread is 0.03 * |W0 row|: most channels have |mu| beyond 30 sigma.  Same bars, same gradient protocol."""
    case = bc.make_case(64, 200, 777, h_shift=1.0, h_scale=0.02)
    h, edges, ws, bs = case[:4]
    mu, var = bc.statistics(h.double(), edges, [w.double() for w in ws], [b.double() for b in bs])
    far = int((mu.abs() >= 30 * torch.sqrt(var + EPS)).sum())
    print(f"\nshifted mean: {far} of 64 channels with |mu| >= 30 sigma")
    assert far >= 8
    _check_case(eps, dev, f"shifted mean masks={masked}", case, masked)


def test_more_tiles_than_workgroups(eps, dev):
    """The statistics pass, the forward and the grad gamma pass run two workgroups per CU, the dy and dz passes one: with more
    than 2 x CUs tiles every workgroup walks several, and the triples and column sums it keeps across its tiles are in play.
    H = 64, masks on."""
    B = 64 * 2 * torch.cuda.get_device_properties(dev).multi_processor_count + 65
    _check_case(eps, dev, f"H=64 B={B} persistent", bc.make_case(64, B, 99), True)


def test_two_calls_return_the_same_bits(eps, dev):
    case = bc.make_case(64, 4096, 11)
    d = _to_dev(case, dev)
    kw = eps.ops.pack_mask(case[6].to(dev)).unsqueeze(0).contiguous()
    a, b = _hip_step(eps, d, kw, 2.0), _hip_step(eps, d, kw, 2.0)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k]), k
    assert bool(a[4]["h"].abs().max() > 0) and bool(a[4]["w0"].abs().max() > 0)


def test_through_the_model(eps, dev, monkeypatch):
    """tests/test_gpu_dea.py::_training_step_vs_truth's construction at H = 32 with the fused decode on: logits, every
    parameter's gradient (the embedding and the TAG layers included) and the running statistics against float64, to that
    function's gates."""
    from eps_amd import models, synth
    adj = synth.rmat_graph(8, 6, 4, "cpu").to(dev)
    torch.manual_seed(0)
    n, H, fin = adj.n_rows, 32, 12
    m = models.DEA_GNN_JK(n, H, H + fin, H, H, 3, H, H, 1, 2, 0.0, True, True, 2, "max").to(dev).train()
    x = torch.randn(n, fin, device=dev)
    edges = torch.randint(0, n, (2, 300), device=dev)
    label = torch.cat([torch.ones(150), torch.zeros(150)]).to(dev)
    p64 = {k: v.detach().double().clone().requires_grad_(v.dtype.is_floating_point and "running" not in k)
           for k, v in m.state_dict().items()}
    p32 = tt.params_as(m, torch.float32, buffers=True)

    # off (the default): the torch route; the new ops are never reached
    def boom(*a, **k):
        raise AssertionError("fused op called with fused_decode off")

    state = {k: v.clone() for k, v in m.state_dict().items()}
    with monkeypatch.context() as mp:
        for name in ("mlp_decode_bn_stats", "mlp_decode_bn_backward", "mlp_decode_train"):
            mp.setattr(eps.ops, name, boom)
        m.loss(m(x, edges, adj), label).backward()
    assert all(p.grad is not None for p in m.parameters())
    m.zero_grad(set_to_none=True)
    m.load_state_dict(state)                       # (the torch step moved the running statistics)
    assert int(m.mlp_bns[0].num_batches_tracked) == 0

    m.eval()
    h_before = m.embeddings(x, adj)
    assert m.embeddings(x, adj) is h_before
    m.train()
    m.fused_decode = True
    versions = (m.mlp_bns[0].running_mean._version, m.mlp_bns[0].running_var._version)
    out = m(x, edges, adj)
    m.loss(out, label).backward()
    assert int(m.mlp_bns[0].num_batches_tracked) == 1
    assert m.mlp_bns[0].running_mean._version > versions[0] and m.mlp_bns[0].running_var._version > versions[1]
    m.eval()
    assert m.embeddings(x, adj) is not h_before    # recomputed: the buffers' versions moved
    m.train()

    ref = tt.dea_forward(p64, tt.dense_adjacency(adj, torch.float64, dev), x, edges, "max")
    assert float((ref.detach() - out.detach().double()).abs().max()) <= 1e-4 * max(1.0, float(ref.detach().abs().max()))
    tt.bce_logits_loss(ref, label).backward()
    tt.bce_logits_loss(tt.dea_forward(p32, tt.dense_adjacency(adj, torch.float32, dev), x, edges, "max"), label).backward()
    worst = 0.0
    for k, p in m.named_parameters():
        scale = max(1e-4, float(p64[k].grad.abs().max()))
        err = float((p.grad.double() - p64[k].grad).abs().max())
        worst = max(worst, err / (2e-4 * scale))
        if err > 2e-4 * scale:
            d32 = float((p32[k].grad.double() - p64[k].grad).abs().max())
            print(f"\ndea fused: {k} past the 2e-4 gate ({err / (2e-4 * scale):.3f}); |hip - f64| / |f32 dense - f64| = "
                  f"{err / max(d32, 1e-300):.2f}")
            assert err <= 4.0 * d32, (k, err, scale, d32)
    print(f"\ndea fused: largest gradient error / gate = {worst:.3f}")
    assert int(torch.count_nonzero(m.lins[0].bias.grad)) == 0
    for k, b in m.named_buffers():
        if "running" in k:
            assert float((b.double() - p64[k]).abs().max()) <= 1e-5 * max(1.0, float(p64[k].abs().max())), k


def test_model_refuses_what_the_kernels_do_not_take(eps, dev):
    from eps_amd import models
    h = torch.zeros(4, 32, device=dev)
    m = models.DEA_GNN_JK(4, 32, 32, 32, 32, 3, 32, 32, 1, 2, 0.0, True, True).to(dev).train()
    with pytest.raises(ValueError, match="B=1"):
        m.decode_train(h, torch.zeros(2, 1, dtype=torch.long, device=dev))
    for kw in (dict(mlp_num_layers=3, mlp_batchnorm=True), dict(mlp_num_layers=2, mlp_batchnorm=False)):
        m = models.DEA_GNN_JK(4, 32, 32, 32, 32, 3, 32, 32, 1, dropout=0.0, gnn_batchnorm=True, **kw).to(dev).train()
        with pytest.raises(ValueError, match="outside the kernel's domain"):
            m.decode_train(h, torch.zeros(2, 3, dtype=torch.long, device=dev))
    # the library itself: EPS_EINVAL names the value, before any launch
    ws = [torch.zeros(32, 32, device=dev), torch.zeros(1, 32, device=dev)]
    bs = [torch.zeros(32, device=dev), torch.zeros(1, device=dev)]
    u = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(eps.EpsError, match="n_pairs=1"):
        eps.ops.mlp_decode_bn_stats(h, u, u, ws, bs)


def test_rank_cli_trains_with_the_fused_decode(eps, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.08")
    from eps_amd import filter_stage, models, rank_stage, training
    losses, calls = [], []
    orig, orig_dt = training.train, models.DEA_GNN_JK.decode_train

    def spy(*a, **k):
        losses.append(orig(*a, **k))
        return losses[-1]

    def counted(self, h, edges):
        calls.append(edges.shape[1])
        return orig_dt(self, h, edges)

    monkeypatch.setattr(rank_stage, "train", spy)
    monkeypatch.setattr(models.DEA_GNN_JK, "decode_train", counted)
    torch.manual_seed(1)
    curves = rank_stage.main(["--dataset", "ddi", "--model", "dea", "--synthetic", "--fused_decode_bn", "--hidden_channels", "32",
                              "--batch_size", "4096", "--epochs", "6", "--runs", "1", "--save_models"])
    assert len(losses) == 6 and all(np.isfinite(losses)) and min(losses[-2:]) < losses[0] - 0.02, losses
    assert calls, "the fused decode was never used"
    assert len(curves) == 1
    assert os.listdir("models") == ["ddi_dea||0|0.pt"]
    fname = filter_stage.main(["--dataset", "ddi", "--model", "dea", "--checkpoint", "ddi_dea||0|0.pt", "--synthetic",
                               "--hidden_channels", "32", "--keep_top", "1000"])
    got = torch.load(fname)
    assert got.shape == (1000, 3) and bool((got[:-1, 2] >= got[1:, 2]).all())
