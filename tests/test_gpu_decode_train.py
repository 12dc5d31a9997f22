"""GPU: the fused training decode (csrc/mlp_decode_train.hip; ops.mlp_decode_train / mlp_decode_backward; LinkGNN.fused_decode;
rank.py --fused_decode) against the float64 restatement of tests/training_truth.py.  N = 50 nodes, so endpoints collide; every
batch holds a self pair and a duplicated pair; B crosses the 64-edge tile, H = 36 takes the pad columns, 256 is the full tile."""
import ctypes
import os

import numpy as np
import pytest
import torch

import decode_train_cases as dc
import training_truth as tt

pytestmark = pytest.mark.gpu

SHAPES = [(H, L, B) for H in (36, 64, 256) for L in (2, 3) for B in (1, 63, 64, 65, 200)]


def _seed(H, L, B):
    return 1000 * H + 10 * B + L


def _dev_case(H, L, B, dev):
    h, edges, ws, bs, keep = dc.make_case(H, L, B, _seed(H, L, B))
    d = dict(h=h.to(dev), u=edges[0].to(dev, torch.int32), v=edges[1].to(dev, torch.int32), ws=[w.to(dev) for w in ws],
             bs=[b.to(dev) for b in bs])
    return (h, edges, ws, bs, keep), d


@pytest.mark.parametrize("H,L,B", SHAPES)
def test_forward_scores_and_taken_bits(eps, dev, H, L, B):
    (h, edges, ws, bs, keep), d = _dev_case(H, L, B, dev)
    ops = eps.ops
    # without masks: the inference kernel's bits, with and without the taken output
    plain = ops.mlp_decode(d["h"], d["u"], d["v"], d["ws"], d["bs"])
    assert torch.equal(ops.mlp_decode_train(d["h"], d["u"], d["v"], d["ws"], d["bs"]), plain)
    out0, taken0 = ops.mlp_decode_train(d["h"], d["u"], d["v"], d["ws"], d["bs"], want_taken=True)
    assert torch.equal(out0, plain)
    f64 = lambda xs: [x.double() for x in xs]   # noqa: E731
    for kp, scale, out, taken in [(None, 1.0, out0, taken0),
                                  (keep, 2.0) + tuple(ops.mlp_decode_train(d["h"], d["u"], d["v"], d["ws"], d["bs"],
                                                                            keep=ops.pack_mask(keep.to(dev)), keep_scale=2.0,
                                                                            want_taken=True))]:
        pre = []
        ref = dc.decode_forward(h.double(), edges, f64(ws), f64(bs), kp, scale, pre=pre)
        err = float((out.double().cpu() - ref).abs().max())
        print(f"\nH={H} L={L} B={B} masks={kp is not None}: max |hip - f64| = {err:.3g}")
        assert err <= 1e-5
        got = ops.unpack_mask(taken, H).cpu()
        assert tuple(got.shape) == (L - 1, B, H)
        for l, z in enumerate(pre):
            differ = (z > 0) != got[l]
            if bool(differ.any()):
                assert float(z[differ].abs().max()) <= 1e-5 * max(1.0, float(z.abs().max()))


def _hip_grads(ops, d, keep_words, scale):
    out, taken = ops.mlp_decode_train(d["h"], d["u"], d["v"], d["ws"], d["bs"], keep=keep_words, keep_scale=scale, want_taken=True)
    leaf = out.clone().requires_grad_(True)
    dc.loss_of(leaf).backward()
    gh, gw, gb = ops.mlp_decode_backward(d["h"], d["u"], d["v"], d["ws"], d["bs"], leaf.grad.contiguous(), keep=keep_words,
                                         keep_scale=scale)
    got = {"h": gh}
    got.update({f"w{i}": g for i, g in enumerate(gw)})
    got.update({f"b{i}": g for i, g in enumerate(gb)})
    return got, taken


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,L,B", SHAPES)
def test_gradients_match_float64(eps, dev, H, L, B, masked):
    (h, edges, ws, bs, keep), d = _dev_case(H, L, B, dev)
    kp, scale = (keep, 2.0) if masked else (None, 1.0)
    got, taken = _hip_grads(eps.ops, d, eps.ops.pack_mask(keep.to(dev)) if masked else None, scale)
    branch = list(eps.ops.unpack_mask(taken, H).cpu())
    g64 = dc.reference_grads(h, edges, ws, bs, kp, scale, branch, torch.float64)
    g32 = dc.reference_grads(h, edges, ws, bs, kp, scale, branch, torch.float32)
    assert set(got) == set(g64) and all(tuple(got[k].shape) == tuple(g64[k].shape) for k in got)
    dc.check_grads(f"H={H} L={L} B={B} masks={masked}", got, g64, g32)


def test_more_tiles_than_workgroups(eps, dev):
    """Both launches are persistent (two workgroups per CU forward, one backward): with more than 2 x CUs tiles every workgroup
    walks several, and the column sums it keeps across its tiles are in play.  H = 64, L = 3, masks on."""
    H, L = 64, 3
    B = 64 * 2 * torch.cuda.get_device_properties(dev).multi_processor_count + 65
    (h, edges, ws, bs, keep), d = _dev_case(H, L, B, dev)
    kw = eps.ops.pack_mask(keep.to(dev))
    got, taken = _hip_grads(eps.ops, d, kw, 2.0)
    out = eps.ops.mlp_decode_train(d["h"], d["u"], d["v"], d["ws"], d["bs"], keep=kw, keep_scale=2.0)
    ref = dc.decode_forward(h.double(), edges, [w.double() for w in ws], [b.double() for b in bs], keep, 2.0)
    assert float((out.double().cpu() - ref).abs().max()) <= 1e-5
    branch = list(eps.ops.unpack_mask(taken, H).cpu())
    g64 = dc.reference_grads(h, edges, ws, bs, keep, 2.0, branch, torch.float64)
    g32 = dc.reference_grads(h, edges, ws, bs, keep, 2.0, branch, torch.float32)
    dc.check_grads(f"H={H} L={L} B={B} persistent", got, g64, g32)


def test_backward_and_dropout_are_reproducible(eps, dev):
    H, L, B, n = 64, 3, 4096, 8
    g = torch.Generator().manual_seed(11)
    h = torch.randn(n, H, generator=g).to(dev)
    u, v = (torch.randint(0, n, (B,), generator=g).to(dev, torch.int32) for _ in range(2))
    ws = [torch.randn(H, H, generator=g).to(dev) / 8 for _ in range(L - 1)] + [torch.randn(1, H, generator=g).to(dev) / 8]
    bs = [torch.randn(H, generator=g).to(dev) / 8 for _ in range(L - 1)] + [torch.randn(1, generator=g).to(dev)]
    go = torch.randn(B, generator=g).to(dev)
    keep = eps.ops.pack_mask(torch.rand(L - 1, B, H, generator=g).to(dev) >= 0.5)
    runs = [eps.ops.mlp_decode_backward(h, u, v, ws, bs, go, keep=keep, keep_scale=2.0) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and bool(runs[0][0].abs().max() > 0)
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)
    from eps_amd import models
    torch.manual_seed(3)
    lp = models.LinkPredictor(H, H, 1, L, 0.5).to(dev).train()
    edges = torch.stack([u, v]).long()
    outs = []
    for _ in range(2):
        torch.manual_seed(17)
        outs.append(lp.decode_train(h, edges).detach())
    assert torch.equal(outs[0], outs[1])
    torch.manual_seed(18)
    assert not torch.equal(lp.decode_train(h, edges).detach(), outs[0])       # (the masks do come from the generator)


def _graph(eps, dev, n=300, m=2000, seed=5):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    ok = u != v
    ei = torch.from_numpy(np.stack([np.r_[u[ok], v[ok]], np.r_[v[ok], u[ok]]]))
    return eps.CSRGraph.from_edge_index(ei, torch.ones(ei.shape[1]), (n, n)).fill_value(1.0).to(dev)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_through_the_model(eps, dev, kind, monkeypatch):
    from eps_amd import models
    adj = _graph(eps, dev)
    n, H, n_pos = adj.n_rows, 64, 300
    torch.manual_seed(3)
    cls = models.GCN if kind == "gcn" else models.SAGE
    model = models.LinkGNN(torch.nn.Embedding(n, H), cls(H, H, H, 3, 0.0), models.LinkPredictor(H, H, 1, 3, 0.0)).to(dev).train()
    gen = torch.Generator().manual_seed(4)
    row, col, _ = adj.cpu().coo()
    pick = torch.randint(0, row.numel(), (n_pos,), generator=gen)
    edges = torch.cat([torch.stack([row[pick], col[pick]]), torch.randint(0, n, (2, n_pos), generator=gen)], 1).to(dev)

    # off (the default): the torch route; the new op is never reached
    def boom(*a, **k):
        raise AssertionError("fused op called with fused_decode off")

    with monkeypatch.context() as mp:
        mp.setattr(eps.ops, "mlp_decode_train", boom)
        off = model(None, edges, adj).squeeze(1)
        tt.log_loss(off, n_pos).backward()
    assert all(p.grad is not None for p in model.parameters())
    model.zero_grad(set_to_none=True)

    model.fused_decode = True
    taken, hs = [], []
    hooks = [m.register_forward_hook(lambda mod, inp, o: taken.append(o.detach() > 0)) for m in model.gnn.convs[:-1]]
    hooks.append(model.gnn.register_forward_hook(lambda mod, inp, o: hs.append(o.detach())))
    out = model(None, edges, adj).squeeze(1)
    for hk in hooks:
        hk.remove()
    tt.log_loss(out, n_pos).backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    ws, bs = model.linkpred._decoder_layers()
    e32 = edges.to(torch.int32)
    _, bits = eps.ops.mlp_decode_train(hs[0].contiguous(), e32[0].contiguous(), e32[1].contiguous(), ws, bs, want_taken=True)
    taken += list(eps.ops.unpack_mask(bits, H))
    assert len(taken) == 4
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = tt.params_as(model, dt)
        o = tt.link_gnn_forward(kind, p, tt.dense_adjacency(adj, dt, dev), tt.dense_pattern(adj, dt, dev), None, edges, branch=taken)
        tt.log_loss(o, n_pos).backward()
        ref[dt] = (o.detach(), {k: v.grad for k, v in p.items()})
    assert float((out.detach().double() - ref[torch.float64][0]).abs().max()) < 1e-5
    dc.check_grads(f"model/{kind}", grads, ref[torch.float64][1], ref[torch.float32][1])


@pytest.mark.parametrize("H,L,word", [(20, 2, "hdim=20"), (260, 2, "hdim=260"), (64, 1, "n_layers=1")])
def test_unsupported_shapes_are_errors_before_any_launch(eps, dev, H, L, word):
    n = 8
    h = torch.zeros(n, H, device=dev)
    ws = [torch.zeros(H, H, device=dev) for _ in range(L - 1)] + [torch.zeros(1, H, device=dev)]
    bs = [torch.zeros(H, device=dev) for _ in range(L - 1)] + [torch.zeros(1, device=dev)]
    u = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(eps.EpsError, match=word) as ei:
        eps.ops.mlp_decode_train(h, u, u, ws, bs)
    assert "eps_mlp_decode_train" in str(ei.value)
    with pytest.raises(eps.EpsError, match=word) as ei:
        eps.ops.mlp_decode_backward(h, u, u, ws, bs, torch.zeros(4, device=dev))
    assert "eps_mlp_decode_backward" in str(ei.value)
    # the same through the C ABI with buffers of our own: EPS_EINVAL, and the buffers keep their fill
    out = torch.full((4,), 7.0, device=dev)
    gh = torch.full((n, H), 7.0, device=dev)
    wp = (ctypes.c_void_p * L)(*[w.data_ptr() for w in ws])
    bp = (ctypes.c_void_p * L)(*[b.data_ptr() for b in bs])
    torch.cuda.synchronize()
    lib = eps.load()
    rc = lib.eps_mlp_decode_train(h.data_ptr(), n, H, u.data_ptr(), u.data_ptr(), 4, wp, bp, L, None, 1.0, 0, out.data_ptr(), None, None)
    assert rc == -1 and word.encode() in lib.eps_last_error()
    rc = lib.eps_mlp_decode_backward(h.data_ptr(), n, H, u.data_ptr(), u.data_ptr(), 4, wp, wp, bp, L, None, 1.0, 0, out.data_ptr(),
                                     None, None, None, None, gh.data_ptr(), None, 0, None)
    torch.cuda.synchronize()
    assert rc == -1 and word.encode() in lib.eps_last_error()
    assert bool((out == 7.0).all()) and bool((gh == 7.0).all())


def test_width_outside_the_domain_is_a_value_error_not_a_fallback(eps, dev):
    from eps_amd import models
    lp = models.LinkPredictor(20, 20, 1, 2, 0.0).to(dev).train()
    with pytest.raises(ValueError, match="outside the kernel's domain"):
        lp.decode_train(torch.zeros(4, 20, device=dev), torch.zeros(2, 3, dtype=torch.long, device=dev))


def test_rank_cli_trains_with_the_fused_decode(eps, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.08")
    from eps_amd import filter_stage, models, rank_stage, training
    losses, calls = [], []
    orig, orig_dt = training.train, models.LinkPredictor.decode_train

    def spy(*a, **k):
        losses.append(orig(*a, **k))
        return losses[-1]

    def counted(self, h, edges):
        calls.append(edges.shape[1])
        return orig_dt(self, h, edges)

    monkeypatch.setattr(rank_stage, "train", spy)
    monkeypatch.setattr(models.LinkPredictor, "decode_train", counted)
    torch.manual_seed(1)
    curves = rank_stage.main(["--dataset", "ddi", "--model", "gcn", "--runs", "1", "--epochs", "6", "--synthetic", "--fused_decode",
                              "--hidden_channels", "32", "--batch_size", "4096", "--save_models", "--eval_steps", "3"])
    assert len(losses) == 6 and all(np.isfinite(losses)) and min(losses[1:]) < losses[0], losses
    assert calls, "the fused decode was never used"
    assert len(curves) == 1
    assert os.listdir("models") == ["ddi_gcn||0|0.pt"]
    fname = filter_stage.main(["--dataset", "ddi", "--model", "gcn", "--checkpoint", "ddi_gcn||0|0.pt", "--synthetic",
                               "--hidden_channels", "32", "--keep_top", "1000"])
    got = torch.load(fname)
    assert got.shape == (1000, 3) and bool((got[:-1, 2] >= got[1:, 2]).all())
