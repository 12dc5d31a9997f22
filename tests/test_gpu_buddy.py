"""GPU: heuristics.sketch_pair_counts / sketch_features against the numpy restatement of tests/sketch_truth.py (and bit for bit
against the same torch formulas on the truth's integer statistics), BuddyLinkModel's train- and eval-mode scores and gradients
against the float64 dense restatement, its eval scores' symmetry, batch independence and both caches, one training epoch, and
rank.py / filter.py --model buddy through their command lines."""
import argparse
import os

import numpy as np
import pytest
import torch

import sketch_truth as st
import test_gpu_training as tgt
import training_truth as tt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(eps, dev):
    """A 300-node skewed symmetric graph, on the device and as scipy, with its truth tables."""
    A = st.skewed_graph(n=300, m=1500, seed=2)
    g = eps.CSRGraph.from_scipy(A, device=dev)
    assert g.val is None and g.n_rows == 300
    return dict(A=A, g=g, tabs=st.tables(A, 2))


@pytest.mark.parametrize("hops", [1, 2])
def test_features_equal_the_formulas_on_the_truth_statistics(eps, dev, small, hops):
    """Against the numpy restatement (estimator and formulas, to the ulps of the platform's log / log1p); and, equal integers in,
    the same torch function on the same device: equal bits out."""
    from eps_amd import heuristics
    A, g = small["A"], small["g"]
    n = A.shape[0]
    rng = np.random.default_rng(9)
    u, v = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    u[:5], v[:5] = [0, 1, 2, 3, 4], [0, 0, 2, 299, 4]
    hll, mh = small["tabs"][0][:hops], small["tabs"][1][:hops]
    S, Z, M = (torch.from_numpy(x).to(dev) for x in st.pair_stats(hll, mh, u, v))
    h = hll.astype(np.int64)
    card = heuristics.sketch_cardinality(torch.from_numpy((np.int64(1) << (33 - h)).sum(-1)).to(dev), torch.from_numpy((h == 0).sum(-1)).to(dev))
    ut, vt = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    I = heuristics.sketch_intersections(S, Z, M)
    want = heuristics.sketch_feature_formulas(I, card[:, ut], card[:, vt])
    e = torch.stack([ut, vt])
    got = heuristics.sketch_features(g, e, hops)
    assert got.dtype == torch.float32 and got.shape == (3000, 5 if hops == 2 else 2) and not got.requires_grad
    assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0
    assert torch.equal(heuristics.sketch_pair_counts(g, e, hops), I)
    assert torch.equal(g.sketches(hops)[2], card)
    # ... and against the numpy restatement of the estimator and of the five formulas.  The float64 operations are the same IEEE
    # ones but for the platform's log / log1p: I within 4 ulp of float64; F within 2 ulp of float32, plus 1e-10 absolute: where
    # the differences of a formula cancel, an ulp of the log in I (1e-13 at these magnitudes) is left as an ABSOLUTE error
    wI, wF = st.pair_features(hll, mh, u, v)
    gI = I.cpu().numpy()
    assert np.array_equal(gI.shape, wI.shape) and bool((np.abs(gI - wI) <= 4 * np.spacing(np.abs(wI))).all())
    gF = got.cpu().numpy()
    errF = np.abs(gF.astype(np.float64) - wF.astype(np.float64))
    print(f"\nhops {hops}: features, max |hip - numpy| in float32 ulps of the value: "
          f"{float((errF / np.spacing(np.maximum(np.abs(wF), np.float32(1e-30)))).max()):.2f}; columns' maxima {wF.max(0)}")
    assert gF.shape == wF.shape and bool((errF <= 2 * np.spacing(np.abs(wF)).astype(np.float64) + 1e-10).all())
    assert bool((wF.max(0) > 0.5).all())                                       # every feature is exercised away from the clamp
    assert np.allclose(g.sketches(hops)[2].cpu().numpy(), st.row_cardinality(hll), rtol=1e-14, atol=0)
    # swapping the endpoints gives the same bits
    assert torch.equal(heuristics.sketch_features(g, e.flip(0), hops), got)
    assert torch.equal(heuristics.sketch_pair_counts(g, e.flip(0), hops), I.transpose(1, 2))
    # the estimates follow the exact counts (the truth's accuracy is the host test's matter): I_11 against CN
    exact = st.exact_intersections(st.exact_sets(A, hops), u, v)[:, 0, 0]
    assert np.corrcoef(I[:, 0, 0].cpu().numpy(), exact)[0, 1] > 0.8
    with pytest.raises(eps.EpsError, match="node ids"):
        heuristics.sketch_features(g, torch.tensor([[0], [n]]), hops)
    assert heuristics.sketch_features(g, torch.zeros((2, 0), dtype=torch.long), hops).shape == (0, 5 if hops == 2 else 2)


@pytest.mark.parametrize("hops", [1, 2])
def test_eval_scores_symmetry_batches_and_caches(eps, dev, small, hops, monkeypatch):
    from eps_amd import models
    g, n, H = small["g"], 300, 32
    torch.manual_seed(3)
    model = models.BuddyLinkModel(torch.nn.Embedding(n, H), H + 6, H, 3, 0.0, hops=hops).to(dev).eval()
    x = torch.randn(n, 6, generator=torch.Generator().manual_seed(4)).to(dev)
    monkeypatch.setattr(models, "NCN_EVAL_TILE", 256)                          # (a tile boundary inside a small batch)
    e = torch.randint(0, n, (2, 700), generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        a = model(x, e, g)
        assert a.shape == (700, 1) and a.dtype == torch.float32 and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
        assert len(torch.unique(a)) > 300
        assert torch.equal(model(x, e.flip(0), g), a)                          # score(u, v) == score(v, u)
        # alone, in a batch of 5, and in a batch that crosses a tile boundary
        assert torch.equal(model(x, e[:, 300:301], g), a[300:301])
        assert torch.equal(model(x, e[:, 298:303], g), a[298:303])
        assert torch.equal(model(x, e[:, 250:262], g), a[250:262])
        assert torch.equal(torch.cat([model(x, e[:, :301], g), model(x, e[:, 301:], g)]), a)
        # the embedding cache is rebuilt after a parameter changes
        h0 = model.embeddings(x, g)
        assert model.embeddings(x, g) is h0
        model.feat_lin.bias.add_(0.25)
        h1 = model.embeddings(x, g)
        assert h1 is not h0 and not torch.equal(h1, h0)
        b = model(x, e, g)
        assert not torch.equal(b, a)
        # the sketch cache belongs to the graph: with_edges gives a new uid, new tables and other scores
        hub = int(torch.argmax(g.degree()))
        extra = torch.stack([torch.full((40,), hub), torch.arange(40)]).to(dev)
        g2 = g.with_edges(extra, False)
        assert g2.uid != g.uid and ("sketch", hops) not in g2._cache and ("sketch", hops) in g._cache
        c = model(x, e, g2)
        assert ("sketch", hops) in g2._cache and not torch.equal(g2.sketches(hops)[0], g.sketches(hops)[0])
        assert c.shape == b.shape and not torch.equal(c, b)
        assert torch.equal(model(x, e, g), b)                                  # and the first graph's scores are served again


@pytest.mark.parametrize("hops,fin", [(1, 0), (2, 6)])
def test_model_against_the_dense_restatement(eps, dev, small, hops, fin):
    """BuddyLinkModel (3 decoder layers, dropout 0, H = 32) on the 300-node graph, with features (embedding first) and without:
    the train-mode scores, every parameter's gradient and the eval-mode scores against the float64 dense restatement
    ``sketch_truth.buddy_forward`` fed the TRUTH's numpy features, under the rules of tests/test_gpu_ncn.py::test_model_gradients:
    scores within max(1e-5, 4 x the float32 dense formulation's own distance from float64), gradients by
    test_gpu_training._check_grads on the branch the HIP forward took."""
    from eps_amd import models
    g, A, n, H = small["g"], small["A"], 300, 32
    torch.manual_seed(11)
    model = models.BuddyLinkModel(torch.nn.Embedding(n, H), H + fin, H, 3, 0.0, hops=hops).to(dev)
    x = torch.randn(n, fin, generator=torch.Generator().manual_seed(12)).to(dev) if fin else None
    n_pos = 512
    edges = tgt._edge_batch(g, n_pos, torch.Generator().manual_seed(4)).to(dev)
    e_np = edges.cpu().numpy()
    feats = torch.from_numpy(st.pair_features(small["tabs"][0][:hops], small["tabs"][1][:hops], e_np[0], e_np[1])[1]).to(dev)
    model.train()
    taken, lp = [], model.linkpred
    hooks = [m.register_forward_hook(lambda mod, inp, o: taken.append(o.detach() > 0)) for m in [lp.xij_lin, lp.xs_lin] + list(lp.lins[:-1])]
    out = model(x, edges, g).squeeze(1)
    for hk in hooks:
        hk.remove()
    tt.log_loss(out, n_pos).backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(v is not None for v in grads.values()) and len(taken) == 3
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = tt.params_as(model, dt)
        Ad = tt.dense_adjacency(g, dt, dev)
        with torch.no_grad():
            free = st.buddy_forward(p, Ad, x, edges, feats, hops)                 # its own ReLU branches: what eval is held to
        o = st.buddy_forward(p, Ad, x, edges, feats, hops, branch=taken)
        tt.log_loss(o, n_pos).backward()
        ref[dt] = (o.detach(), {k: v.grad for k, v in p.items()}, free)
    f32_err = float((ref[torch.float32][0].double() - ref[torch.float64][0]).abs().max())
    out_err = float((out.detach().double() - ref[torch.float64][0]).abs().max())
    model.eval()
    with torch.no_grad():
        ev = model(x, edges, g).squeeze(1)
    f32_free = float((ref[torch.float32][2].double() - ref[torch.float64][2]).abs().max())
    ev_err = float((ev.double() - ref[torch.float64][2]).abs().max())
    print(f"\nbuddy hops={hops} fin={fin}: train scores max |hip - f64| = {out_err:.3g} (f32 dense {f32_err:.3g}); "
          f"eval scores {ev_err:.3g} (f32 dense {f32_free:.3g}); score range [{float(ev.min()):.3f}, {float(ev.max()):.3f}]")
    assert float(ev.max()) - float(ev.min()) > 0.05
    assert out_err <= max(1e-5, 4.0 * f32_err)
    assert ev_err <= max(1e-5, 4.0 * f32_free)
    tgt._check_grads(f"buddy hops={hops} fin={fin}", grads, ref[torch.float64][1], ref[torch.float32][1], floor=1e-6)


def test_one_training_epoch(eps, dev, small):
    from eps_amd import models, training
    g, A, n, H = small["g"], small["A"], 300, 32
    torch.manual_seed(7)
    model = models.BuddyLinkModel(torch.nn.Embedding(n, H), H, H, 3, 0.1, hops=2).to(dev)
    coo = A.tocoo()
    keep = coo.row < coo.col
    split_edge = {"train": {"edge": torch.from_numpy(np.stack([coo.row[keep], coo.col[keep]], 1).astype(np.int64))}}
    data = argparse.Namespace(x=None, adj_t=g, num_nodes=n)
    seen = []
    model.linkpred.register_forward_pre_hook(lambda mod, inp: seen.append((inp[2].requires_grad, inp[2].shape, inp[0].requires_grad)))
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    loss = training.train(model, data, "ddi", split_edge, opt, 1 << 20, True, "buddy", dev)
    assert np.isfinite(loss) and loss > 0
    assert len(seen) == 1 and seen[0][0] is False and seen[0][1][1] == 5 and seen[0][2] is True
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    assert "emb.weight" in dict(model.named_parameters())


# ---------------------------------------------------------------------------------------------------------- command lines
@pytest.fixture(scope="module")
def trained(eps, dev, tmp_path_factory):
    """rank.py --dataset ddi --model buddy --synthetic --epochs 1 --runs 1 on the 0.08 stand-in, once."""
    from eps_amd import rank_stage
    work = tmp_path_factory.mktemp("buddy_cli")
    mp = pytest.MonkeyPatch()
    try:
        mp.chdir(work)
        mp.setenv("EPS_SYNTH_SCALE", "0.08")
        torch.manual_seed(1)
        curves = rank_stage.main(["--dataset", "ddi", "--model", "buddy", "--synthetic", "--hidden_channels", "32", "--epochs", "1",
                                  "--runs", "1", "--batch_size", "4096", "--save_models"])
    finally:
        mp.undo()
    return dict(dir=work, curves=curves)


def test_rank_cli_completes(trained):
    curves = trained["curves"]
    assert len(curves) == 1 and 0.0 <= float(curves[0][1]) <= 100.0 and 0.0 <= float(curves[0][2]) <= 100.0
    assert [f for f in os.listdir(trained["dir"] / "models") if f.startswith("ddi_buddy")] == ["ddi_buddy||0|0.pt"]


def test_filter_cli_equals_the_restatement(eps, dev, trained, monkeypatch):
    """filter.py --model buddy from the saved checkpoint, --keep_top and --keep_per_node (the block route): the rows are in the
    declared order (score descending, then candidate order) and their scores are the model's forward of those pairs bit for bit
    -- against the filter restated here: every candidate expanded, scored in ONE call, ordered by the declared rule."""
    monkeypatch.chdir(trained["dir"])
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.08")
    from eps_amd import candidates, datasets, filter_stage, graph, models, proposals
    argv = ["--dataset", "ddi", "--model", "buddy", "--checkpoint", "ddi_buddy||0|0.pt", "--synthetic", "--hidden_channels", "32"]
    args = models.default_model_configs(filter_stage.make_parser().parse_args(argv))
    ei, ew, _, data = datasets.get_data(args)
    data = data.to(dev)
    model = models.build_model(args, data, dev)
    assert type(model) is models.BuddyLinkModel and model.hops == 2
    model.load_state_dict(torch.load("models/ddi_buddy||0|0.pt", map_location=dev))
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
    assert bool((got[1:, 2] <= got[:-1, 2]).all())
    with torch.no_grad():
        again = model(data.x, got[:, :2].t().to(torch.int64).to(dev), adj).reshape(-1).cpu()
    assert torch.equal(again, got[:, 2])
    monkeypatch.setattr(candidates, "DEFAULT_BLOCK_PATHS", 20_000)                     # many small candidate blocks
    assert torch.equal(torch.load(filter_stage.main(argv + ["--keep_top", "1000"])), full[:1000])
    assert torch.equal(torch.load(filter_stage.main(argv + ["--keep_per_node", "3"])), per_node)
    with pytest.raises(ValueError, match="no MLP decode"):
        filter_stage.main(argv + ["--keep_top", "1000", "--decode_precision", "bf16"])
