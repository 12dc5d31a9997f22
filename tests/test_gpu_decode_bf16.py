"""GPU: the bf16 screening decode -- eps_f32_to_bf16 against torch's conversion, eps_mlp_decode_bf16 against the float64 emulation
of its rounding points (tests/test_decode_bf16_host.py): exactly on integer inputs (lane maps, tail tiles, row gathers), within
the decode bar on random ones; its error paths; and the filter stage's bf16 route, whose rows must carry fp32 scores."""
import argparse
import os

import numpy as np
import pytest
import torch

from test_decode_bf16_host import bf16_to_f64, emulate_decode_bf16, rne_bf16_bits, same_bf16_bits, special_vector

pytestmark = pytest.mark.gpu


def _i16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16))


def _run_kernel(eps, dev, hb, u, v, ws, bs, apply_sigmoid=False):
    L = len(ws)
    dw = [(_i16(w) if i < L - 1 else torch.from_numpy(w)).to(dev) for i, w in enumerate(ws)]
    db = [torch.from_numpy(b).to(dev) for b in bs]
    out = eps.ops.mlp_decode_bf16(_i16(hb).to(dev), torch.from_numpy(u.astype(np.int32)).to(dev),
                                  torch.from_numpy(v.astype(np.int32)).to(dev), dw, db, apply_sigmoid=apply_sigmoid)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------- (a) conversion
def test_to_bf16_matches_torch_bit_for_bit(eps, dev):
    x = special_vector()
    for vec in [x] + [x[27:27 + n] for n in (1, 63, 64, 65, 4099)]:
        t = torch.from_numpy(vec.copy())
        got = eps.ops.to_bf16(t.to(dev))
        assert got.dtype == torch.int16 and got.shape == t.shape
        assert same_bf16_bits(got.cpu().numpy(), t.to(torch.bfloat16).view(torch.int16).numpy(), vec)
        assert same_bf16_bits(got.cpu().numpy(), t.to(dev).to(torch.bfloat16).view(torch.int16).cpu().numpy(), vec)
        assert np.array_equal(got.cpu().numpy().view(np.uint16), rne_bf16_bits(vec))      # (NaNs included: 0x7FC0)
    m = torch.from_numpy(x[:10000].copy()).reshape(100, 100)
    assert eps.ops.to_bf16(m.to(dev)).shape == (100, 100)
    assert eps.ops.to_bf16(torch.zeros(0, device=dev)).numel() == 0


# ---------------------------------------------------------------------------------------------- (b) exact layout test
N_EXACT = 97


def _integer_case(H, L, seed):
    """Integer-valued h, W, b: h in {-1, 0, 1, 2}, six +-1 entries per hidden weight row (every row and, with 6 H draws, every
    column is used), biases in [-2, 2], a dense last layer in [-3, 3]."""
    rng = np.random.default_rng(seed)
    h = rng.choice(np.array([-1, 0, 0, 1, 1, 2], np.float32), size=(N_EXACT, H))
    ws = []
    for _ in range(L - 1):
        W = np.zeros((H, H), np.float32)
        for c in range(H):
            k = rng.choice(H, size=min(6, H), replace=False)
            W[c, k] = rng.choice(np.array([-1, 1], np.float32), size=k.size)
        ws.append(rne_bf16_bits(W))
    ws.append(rng.integers(-3, 4, size=(1, H)).astype(np.float32))
    bs = [rng.integers(-2, 3, size=H).astype(np.float32) for _ in range(L - 1)] + [rng.integers(-2, 3, size=1).astype(np.float32)]
    return rne_bf16_bits(h), ws, bs


def _pair_list(n, seed):
    """n pairs over N_EXACT nodes with u == v entries and repeated pairs."""
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, N_EXACT, n), rng.integers(0, N_EXACT, n)
    if n > 2:
        u[1], v[1] = v[0], u[0]                   # the mirror of pair 0
        u[n // 2], v[n // 2] = u[0], v[0]         # a repeat
        u[-1], v[-1] = N_EXACT - 1, N_EXACT - 1   # the last node with itself, in the tail tile
        v[::7] = u[::7]
    else:
        v[:] = u
    return u, v


def _intermediates_are_small_integers(hb, u, v, ws, bs):
    """Every value the kernel rounds to bf16 (x0 and the hidden activations) and the last hidden layer's output: an integer of
    magnitude <= 256, so exact in bf16 whatever the order of the sums."""
    h = bf16_to_f64(hb)
    x = h[u] * h[v]
    vals = [x]
    for l in range(len(ws) - 1):
        x = np.maximum(x @ bf16_to_f64(ws[l]).T + bs[l].astype(np.float64), 0)
        vals.append(x)
    return all(bool((a == np.rint(a)).all()) and float(np.abs(a).max()) <= 256 for a in vals), max(float(np.abs(a).max()) for a in vals)


@pytest.mark.parametrize("L", [2, 3, 4])
@pytest.mark.parametrize("H", [16, 48, 256])
def test_integer_inputs_decode_exactly(eps, dev, H, L):
    hb, ws, bs = _integer_case(H, L, 100 * H + L)
    for n in (1, 65, 1000):
        u, v = _pair_list(n, n + L)
        ok, top = _intermediates_are_small_integers(hb, u, v, ws, bs)
        assert ok, f"the test's own inputs leave the exact range: max {top}"
        want, _ = emulate_decode_bf16(hb, u, v, ws, bs)
        assert float(np.abs(want).max()) < 2 ** 24 and bool((want == np.rint(want)).all())
        got = _run_kernel(eps, dev, hb, u, v, ws, bs)
        assert got.shape == (n,) and np.array_equal(got.astype(np.float64), want), (H, L, n, np.nonzero(got != want)[0][:8])
    assert float(np.abs(want).max()) > 0          # (not a test of zeros)


# ---------------------------------------------------------------------------------------------- (c), (d) random inputs
BAR = 1e-5          # the decode bar: relative, scaled by the sum of the magnitudes of the final dot's terms (+ |bias|)
FLIP = 2.0 ** -7    # a pair whose hidden rounding flipped: one bf16 ulp of one activation and then some


def _random_case(H, L, seed, n=500, E=1000):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, H, generator=g).numpy()
    ws = [rne_bf16_bits((torch.randn(H, H, generator=g) / H ** 0.5).numpy()) for _ in range(L - 1)]
    ws.append((torch.randn(1, H, generator=g) / H ** 0.5).numpy())
    bs = [(torch.randn(H if i < L - 1 else 1, generator=g) * 0.1).numpy() for i in range(L)]
    u = torch.randint(0, n, (E,), generator=g).numpy()
    v = torch.randint(0, n, (E,), generator=g).numpy()
    return rne_bf16_bits(h), u, v, ws, bs


@pytest.mark.parametrize("H", [48, 256])
def test_random_two_layers_within_the_decode_bar(eps, dev, H):
    """L = 2: the only rounding to bf16 is the Hadamard one, which is deterministic."""
    hb, u, v, ws, bs = _random_case(H, 2, 7 + H)
    want, tsum = emulate_decode_bf16(hb, u, v, ws, bs)
    cpu32, _ = emulate_decode_bf16(hb, u, v, ws, bs, acc=np.float32)
    assert float((np.abs(cpu32 - want) / tsum).max()) <= BAR          # fp32 accumulation can meet the bar on these inputs
    got = _run_kernel(eps, dev, hb, u, v, ws, bs).astype(np.float64)
    err = np.abs(got - want) / tsum
    print(f"H={H} L=2: max err / sum|terms| = {err.max():.3e} (cpu fp32: {(np.abs(cpu32 - want) / tsum).max():.3e})")
    assert float(err.max()) <= BAR
    prob = _run_kernel(eps, dev, hb, u, v, ws, bs, apply_sigmoid=True).astype(np.float64)
    assert float(np.abs(prob - 1 / (1 + np.exp(-got))).max()) <= 2e-7


@pytest.mark.parametrize("H", [48, 256])
def test_random_three_layers_within_the_decode_bar(eps, dev, H):
    """L = 3: the rounding of the first hidden layer can flip by one bf16 ulp where fp32 and float64 sums straddle a boundary."""
    hb, u, v, ws, bs = _random_case(H, 3, 11 + H)
    want, tsum = emulate_decode_bf16(hb, u, v, ws, bs)

    def limits(x, who):
        err = np.abs(x - want) / tsum
        miss = err > BAR
        print(f"H={H} L=3 {who}: {int(miss.sum())} of {err.size} pairs miss {BAR:g}; max err / sum|terms| = {err.max():.3e}")
        return float(miss.mean()) <= 0.01 and float(err.max()) <= FLIP
    cpu32, _ = emulate_decode_bf16(hb, u, v, ws, bs, acc=np.float32)
    assert limits(cpu32, "cpu fp32")              # the seed and the scale leave room for a correct fp32 accumulation
    got = _run_kernel(eps, dev, hb, u, v, ws, bs).astype(np.float64)
    assert limits(got, "kernel")


# ---------------------------------------------------------------------------------------------- (e) error paths
@pytest.mark.parametrize("H,L,word", [(20, 2, "hdim=20"), (272, 2, "hdim=272"), (256, 1, "n_layers=1")])
def test_unsupported_shapes_are_errors_before_any_launch(eps, dev, H, L, word):
    n = 8
    h = torch.zeros(n, H, dtype=torch.int16, device=dev)
    ws = [torch.zeros(H, H, dtype=torch.int16, device=dev) for _ in range(L - 1)] + [torch.zeros(1, H, device=dev)]
    bs = [torch.zeros(H, device=dev) for _ in range(L - 1)] + [torch.zeros(1, device=dev)]
    u = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(eps.EpsError, match=word) as ei:
        eps.ops.mlp_decode_bf16(h, u, u, ws, bs, apply_sigmoid=False)
    assert "eps_mlp_decode_bf16" in str(ei.value) and word.encode() in eps.load().eps_last_error()
    # the same through the C ABI with an output buffer of our own: the call returns EPS_EINVAL and the buffer keeps its fill
    import ctypes
    out = torch.full((4,), 7.0, device=dev)
    wp = (ctypes.c_void_p * L)(*[w.data_ptr() for w in ws])
    bp = (ctypes.c_void_p * L)(*[b.data_ptr() for b in bs])
    torch.cuda.synchronize()
    rc = eps.load().eps_mlp_decode_bf16(h.data_ptr(), n, H, u.data_ptr(), u.data_ptr(), 4, wp, bp, L, 0, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and word.encode() in eps.load().eps_last_error() and bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------- (f), (g) the filter stage
def _symmetric_graph(eps, dev, n=300, m=2000, seed=5):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = u != v
    ei = torch.from_numpy(np.stack([np.r_[u[keep], v[keep]], np.r_[v[keep], u[keep]]]))
    g = eps.CSRGraph.from_edge_index(ei, torch.ones(ei.shape[1]), (n, n))
    return g.fill_value(1.0).to(dev)


def _link_gnn(n, H, L, seed, dev):
    from eps_amd import models
    torch.manual_seed(seed)
    m = models.LinkGNN(torch.nn.Embedding(n, H), models.GCN(H, H, H, L, 0.0), models.LinkPredictor(H, H, 1, L, 0.0))
    return m.to(dev).eval()


def _small_dea(n, H, seed, dev):
    from eps_amd import models
    torch.manual_seed(seed)
    m = models.DEA_GNN_JK(num_nodes=n, embed_dim=H, gnn_in_dim=H, gnn_hidden_dim=H, gnn_out_dim=H, gnn_num_layers=3, mlp_in_dim=H,
                          mlp_hidden_dim=H, mlp_out_dim=1, mlp_num_layers=2, dropout=0.5, gnn_batchnorm=True, mlp_batchnorm=True)
    g = torch.Generator().manual_seed(seed)
    for bn in list(m.gnn_bns) + list(m.mlp_bns):                   # non-trivial running statistics
        bn.running_mean.copy_(torch.randn(H, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(H, generator=g) + 0.5)
        bn.weight.data.copy_(torch.rand(H, generator=g) + 0.5)
        bn.bias.data.copy_(torch.randn(H, generator=g) * 0.1)
    return m.to(dev).eval()


def _check_rows(eps, model, data, pairs, scores, K):
    """The four properties of a bf16 run's rows: fp32 scores bit for bit, the declared order, no duplicates, no stored edge."""
    g = data.adj_t
    assert pairs.shape == (2, K) and scores.shape == (K,)
    with torch.no_grad():
        fp32 = model(data.x, pairs, g).reshape(-1)
    assert torch.equal(scores, fp32), "a written score is not the fp32 decode of its pair"
    s = scores.cpu().numpy()
    key = (pairs[1].cpu().numpy().astype(np.int64) << 32) | pairs[0].cpu().numpy().astype(np.int64)
    assert bool((s[:-1] >= s[1:]).all())
    tie = s[:-1] == s[1:]
    assert bool((key[:-1][tie] < key[1:][tie]).all()), "equal scores are not in candidate order"
    assert np.unique(key).size == K
    A = g.to_scipy()
    pu, pv = pairs[0].cpu().numpy().copy(), pairs[1].cpu().numpy().copy()          # (scipy indexes with writeable arrays)
    assert not np.asarray(A[pu, pv]).any() and bool((pu != pv).all())
    # (the mirror of a pair carries the same score and sits next to it or at the cut)
    return key


def test_filter_route_is_exact_plumbing(eps, dev):
    from eps_amd import filter_stage
    g = _symmetric_graph(eps, dev)
    model = _link_gnn(g.n_rows, 16, 2, 3, dev)
    data = argparse.Namespace(x=None, adj_t=g, num_nodes=g.n_rows)
    args = argparse.Namespace(model="gcn")
    with torch.no_grad():
        p32, s32, seen32 = filter_stage.gnn_half_topk(args, model, data, 200, 0, 1)
        pb, sb, seenb = filter_stage.gnn_half_topk(args, model, data, 200, 0, 1, precision="bf16", guard=1e9)
    assert seenb == seen32 and seen32 // 2 <= filter_stage.screen_size(200, 1e9)       # M covers every candidate
    assert torch.equal(pb, p32) and torch.equal(sb, s32)
    assert model._hb is not None and model._hb_key == model._h_key                      # the bf16 table sits under h's key
    hb = model._hb
    with torch.no_grad():
        pk, sk, _ = filter_stage.gnn_half_topk(args, model, data, 50, 0, 1, precision="bf16")
    assert model._hb is hb                                                              # ... and is built once
    _check_rows(eps, model, data, pk, sk, 50)
    # a parameter update invalidates both cached copies
    with torch.no_grad():
        model.linkpred.lins[0].weight.mul_(1.5)
        w_old = model.linkpred._bf16_layers[0][0]
        pk2, sk2, _ = filter_stage.gnn_half_topk(args, model, data, 50, 0, 1, precision="bf16")
    assert model.linkpred._bf16_layers[0][0] is not w_old
    _check_rows(eps, model, data, pk2, sk2, 50)


def test_filter_route_dea(eps, dev):
    from eps_amd import filter_stage
    g = _symmetric_graph(eps, dev, seed=6)
    model = _small_dea(g.n_rows, 16, 4, dev)
    data = argparse.Namespace(x=None, adj_t=g, num_nodes=g.n_rows)
    with torch.no_grad():
        pk, sk, _ = filter_stage.gnn_half_topk(argparse.Namespace(model="dea"), model, data, 50, 0, 1, precision="bf16")
    _check_rows(eps, model, data, pk, sk, 50)


def test_filter_cli_bf16(eps, dev, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.15")
    from eps_amd import datasets, filter_stage, models, proposals
    from eps_amd.graph import add_edges
    args = models.default_model_configs(argparse.Namespace(
        dataset="ddi", model="gcn", synthetic=True, num_layers=None, hidden_channels=None, dropout=None, batch_size=None, lr=None,
        epochs=None, use_feature=None, use_learnable_embedding=None))
    edge_index, edge_weight, split_edge, data = datasets.get_data(args)
    torch.manual_seed(0)
    model = models.build_model(args, data, torch.device("cpu"))
    os.makedirs("models", exist_ok=True)
    torch.save(model.state_dict(), "models/ddi_gcn||0|0.pt")
    K = 1000
    argv = ["--dataset", "ddi", "--model", "gcn", "--checkpoint", "ddi_gcn||0|0.pt", "--synthetic", "--keep_top", str(K)]
    fname = filter_stage.main(argv + ["--decode_precision", "bf16"])
    assert os.path.exists(fname)
    rows = proposals.load_sorted_edges(fname)
    assert rows.shape == (K, 3) and rows.dtype == torch.float32
    assert torch.equal(proposals.load_proposals(fname, K), rows[:, :2].t().long())
    data = data.to(dev)
    model = model.to(dev).eval()
    data.adj_t = add_edges("ddi", edge_index.to(dev), edge_weight.to(dev), torch.zeros((2, 0), dtype=torch.long, device=dev),
                           data.num_nodes)
    _check_rows(eps, model, data, rows[:, :2].t().long().to(dev), rows[:, 2].to(dev), K)
    # the same command without the flag: the fp32 route, as before
    plain = torch.load(filter_stage.main(argv))
    with torch.no_grad():
        p32, s32, _ = filter_stage.gnn_half_topk(args, model, data, K, 0, 1)
    assert torch.equal(plain[:, :2].t().long(), p32.cpu()) and torch.equal(plain[:, 2], s32.cpu())
    # membership: what the default guard kept against the fp32 run (reported, not asserted: it is the one thing that may differ)
    a = set(map(tuple, rows[:, :2].long().tolist())); b = set(map(tuple, plain[:, :2].long().tolist()))
    print(f"bf16 run kept {len(a & b)} of the fp32 run's {K} rows")
