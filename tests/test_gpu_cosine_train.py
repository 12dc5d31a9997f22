"""GPU: training through the cosine common-neighbour score ('mlpcos', 'simplecos' with an embedding): the two backward kernels
(csrc/cosine_cn_bwd.hip), the autograd path of CommonNeighborsPredictor, a few Adam steps against a float64 replica, and rank.py
--train_cosine end to end -- all against the float64 truth of test_cosine_train_host.py.  Every check prints its largest
error / bound before it asserts."""
import argparse
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

from conftest import GOLDEN, golden_pair_files
from test_cosine_cn_host import all_pairs_sample, random_graph
from test_cosine_train_host import cosine_grad_truth, grad_tolerance, literal_raw_dense
from test_gpu_cosine_cn import device_graph, features

pytestmark = pytest.mark.gpu


def worst(name, got, truth, tol):
    r = float((np.abs(np.asarray(got, np.float64) - truth) / tol).max())
    print(f"[cosine-train] {name}: largest error / bound = {r:.4f}")
    return r


def forward_pieces(eps, A, x_dev):
    from eps_amd import ops, scan
    g = device_graph(eps, A)
    sym = (abs(ssp.csr_matrix(A) - ssp.csr_matrix(A).T) > 0).nnz == 0
    revpos = scan.reverse_positions(g) if sym else None
    xhat, nrm = ops.cos_node_features(g.rowptr, g.col, g.val, x_dev, want_norm=True)
    assert torch.equal(xhat, ops.cos_node_features(g.rowptr, g.col, g.val, x_dev)), "the norm-returning forward keeps xhat's bits"
    c = ops.edge_cosines(g.rowptr, g.col, xhat, revpos)
    return g, revpos, xhat, nrm, c


def check_pair_backward(eps, A, x_dev, x_np, pairs, gvec, name):
    from eps_amd import ops
    A = ssp.csr_matrix(A)
    A.sort_indices()
    g, _, _, _, c = forward_pieces(eps, A, x_dev)
    u = torch.from_numpy(pairs[0].astype(np.int32)).cuda()
    v = torch.from_numpy(pairs[1].astype(np.int32)).cuda()
    gd = torch.from_numpy(gvec.astype(np.float32)).cuda()
    gc = ops.pair_cn_backward(g.rowptr, g.col, c, u, v, gd)
    again = ops.pair_cn_backward(g.rowptr, g.col, c, u, v, gd)
    assert torch.equal(gc, again), "two runs over the same inputs differ"
    perm = torch.from_numpy(np.random.default_rng(5).permutation(pairs.shape[1])).cuda()
    shuffled = ops.pair_cn_backward(g.rowptr, g.col, c, u[perm].contiguous(), v[perm].contiguous(), gd[perm].contiguous())
    assert torch.equal(gc, shuffled), "the result depends on the order of the pair list"
    t = cosine_grad_truth(A, x_np.astype(np.float64), pairs, gvec.astype(np.float32).astype(np.float64))
    row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    truth, mag = t["gc"][0][row, A.indices], t["gc"][1][row, A.indices]
    got = gc.cpu().numpy()
    assert np.isfinite(got).all()
    f = x_np.shape[1]
    assert worst(f"pair backward {name}", got, truth, grad_tolerance(mag, f, np.abs(gvec).max())) <= 1.0
    touched = mag > 0
    assert not got[~touched].any(), "an entry no pair reaches must stay zero"
    return gc


def special_pairs(n, k, seed):
    """k random pairs + duplicated pairs + u == v pairs (+ whatever has no common neighbour among them)."""
    p = all_pairs_sample(n, k, seed)
    same = np.arange(0, n, max(1, n // 40))
    return np.concatenate([p, p[:, :k // 4], np.stack([same, same])], 1)


@pytest.mark.parametrize("kind", ["unit", "weighted", "selfloop"])
def test_pair_backward_random_graphs(eps, dev, kind):
    n = 300
    A = random_graph(n, 1500, seed=21, weighted=(kind == "weighted"), isolated=5)
    if kind == "selfloop":
        A = ssp.csr_matrix(A + ssp.diags(np.r_[np.zeros(n - 8), np.ones(3), np.zeros(5)]))
    x_dev, x_np = features(n, 24, seed=3)
    pairs = np.concatenate([special_pairs(n, 3000, 4), np.array([[n - 1, n - 2], [0, n - 1]])], 1)    # isolated ends
    gvec = np.random.default_rng(8).standard_normal(pairs.shape[1]) * 0.01
    check_pair_backward(eps, A, x_dev, x_np, pairs, gvec, kind)


@pytest.mark.parametrize("path", golden_pair_files(), ids=lambda p: os.path.basename(p)[6:-4])
def test_pair_backward_golden_graphs(eps, dev, path):
    d = np.load(path)
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((d["val"].astype(np.float64), d["col"], d["rowptr"]), shape=(n, n))
    x_dev, x_np = features(n, 58, seed=n)
    pairs = np.concatenate([d["pairs"], d["pairs"][:, :100], np.stack([np.arange(min(n, 20)), np.arange(min(n, 20))])], 1)
    gvec = np.random.default_rng(n).standard_normal(pairs.shape[1])
    check_pair_backward(eps, A, x_dev, x_np, pairs, gvec, os.path.basename(path))


def test_pair_backward_hub_rows(eps, dev):
    """Rows longer than one LDS stage (> 1024 entries): hub x hub pairs take several staged passes, hub x short-row pairs the
    in-place search."""
    n = 3000
    rng = np.random.default_rng(2)
    r, c = [rng.integers(0, n, 6000)], [rng.integers(0, n, 6000)]
    for hub, deg in ((0, 2200), (1, 1800), (2, 1100)):
        nb = rng.choice(np.arange(3, n), deg, replace=False)
        r.append(np.full(deg, hub)), c.append(nb)
    r, c = np.concatenate(r), np.concatenate(c)
    keep = r != c
    A = ssp.coo_matrix((np.ones(2 * keep.sum()), (np.r_[r[keep], c[keep]], np.r_[c[keep], r[keep]])), shape=(n, n)).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    assert np.diff(A.indptr)[:3].min() > 1024
    x_dev, x_np = features(n, 16, seed=9)
    hubs = np.array([[0, 0, 1, 0, 1, 2, 0, 1, 2], [1, 2, 2, 0, 1, 2, 1, 0, 0]])
    short = np.stack([rng.integers(0, 3, 500), rng.integers(3, n, 500)])
    pairs = np.concatenate([hubs, short, short[::-1], all_pairs_sample(n, 2000, 6)], 1)
    gvec = rng.standard_normal(pairs.shape[1])
    check_pair_backward(eps, A, x_dev, x_np, pairs, gvec, "hub rows")


def switch_point_case(cap, ratio):
    """The boundary graph and pairs of cn_list_truth (rows of 0, 1, 63, 64, 65, cap - 1, cap, cap + 1, 2 cap + 1 entries and an
    in-place hub, every class against every class, u == v), c and g random multiples of 2^-8 in [-1, 1] (some g exactly 0), and
    the SPARSE float64 truth: for every pair and every listed w, at the places e_u, e_v of w in rows u and v,
    gc[e_u] += g c[e_v] and gc[e_v] += g c[e_u].  Checked here, on the CPU: the sums are exact (multiples of 2^-16 below 2^37),
    and one-pass, several-pass and in-place pairs each occur with matches and without."""
    import cn_list_truth as ct
    A, special, stranger = ct.boundary_graph(cap, ratio)
    u, v = ct.boundary_pairs(A, special, stranger)
    ptr, w = ct.cn_lists(A, u, v)
    n, nnz = A.shape[0], A.nnz
    rng = np.random.default_rng(31)
    c = rng.integers(-256, 257, nnz).astype(np.float64) / 256.0
    g = rng.integers(-256, 257, len(u)).astype(np.float64) / 256.0
    g[rng.integers(0, len(u), len(u) // 10)] = 0.0
    g[0] = 1.0                                                                     # (max |g| is known: the scale is 2^46)
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices      # ascending: CSR with sorted rows
    b = np.repeat(np.arange(len(u)), np.diff(ptr))
    eu = np.searchsorted(keys, u[b].astype(np.int64) * n + w)
    ev = np.searchsorted(keys, v[b].astype(np.int64) * n + w)
    assert np.array_equal(A.indices[eu], w) and np.array_equal(A.indices[ev], w)
    truth = np.zeros(nnz, np.float64)
    np.add.at(truth, eu, g[b] * c[ev])
    np.add.at(truth, ev, g[b] * c[eu])                                             # (u == v: the one entry receives both)
    reached = np.zeros(nnz, bool)
    reached[eu] = reached[ev] = True
    assert np.array_equal(truth * 65536.0, np.round(truth * 65536.0)) and np.abs(truth).max() < 2.0 ** 37
    assert (g == 0.0).any() and np.abs(g).max() == 1.0 and not truth[~reached].any()
    deg, cnt = np.diff(A.indptr), np.diff(ptr)
    lo, hi = np.minimum(deg[u], deg[v]), np.maximum(deg[u], deg[v])
    inplace = (hi > cap) & (hi >= lo * ratio) & (lo > 0)
    for path in (inplace, (hi > cap) & ~inplace & (lo > 0), (hi <= cap) & (lo > 0)):
        assert (cnt[path] > 0).any() and (cnt[path] == 0).any()
        assert ((cnt > 0) & path & (g != 0.0)).any()                               # ... and some of the matches carry a gradient
    assert deg[special].tolist() == ct.boundary_lengths(cap, ratio)
    return A, u, v, c.astype(np.float32), g.astype(np.float32), truth, reached


def test_pair_backward_switch_points(eps, dev):
    """The backward at every switch point of its walk (csrc/row_intersect.h), bit for bit.  Every term g c 2^46 is an integer
    (g and c are multiples of 2^-8, the scale is 2^(60 - 12 - 1 - 1) for about 1,100 pairs with max |g| = 1), every fixed-point
    sum is exact, pb_convert_kernel rounds once: gc has the bits of float32(truth), an entry no pair reaches is 0, and the order
    of the list does not matter."""
    from eps_amd import ops
    cap, ratio = ops.pair_cn_list_limits()
    A, u, v, c, g, truth, reached = switch_point_case(cap, ratio)
    rowptr = torch.from_numpy(A.indptr.astype(np.int64)).to(dev)
    col = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
    cd, gd = torch.from_numpy(c).to(dev), torch.from_numpy(g).to(dev)
    ud, vd = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    gc = ops.pair_cn_backward(rowptr, col, cd, ud, vd, gd)
    got, want = gc.cpu().numpy(), truth.astype(np.float32)
    diff = got.view(np.int32) != want.view(np.int32)
    print(f"[cosine-train] switch points: {len(u)} pairs, {A.shape[0]} nodes, {int(reached.sum())} entries reached, "
          f"{int(diff.sum())} entries differ from float32(truth) in their bits")
    assert not diff.any()
    assert not got[~reached].any(), "an entry no pair reaches must stay zero"
    perm = torch.from_numpy(np.random.default_rng(5).permutation(len(u))).to(dev)
    shuffled = ops.pair_cn_backward(rowptr, col, cd, ud[perm].contiguous(), vd[perm].contiguous(), gd[perm].contiguous())
    assert torch.equal(gc.view(torch.int32), shuffled.view(torch.int32)), "the result depends on the order of the pair list"


def test_pair_backward_zero_gradient_and_empty_list(eps, dev):
    from eps_amd import ops
    A = random_graph(100, 400, seed=1)
    x_dev, _ = features(100, 8, seed=1)
    g, _, _, _, c = forward_pieces(eps, A, x_dev)
    u = torch.arange(50, dtype=torch.int32, device="cuda:0")
    assert not ops.pair_cn_backward(g.rowptr, g.col, c, u, u, torch.zeros(50, device="cuda:0")).any()
    e = torch.zeros(0, dtype=torch.int32, device="cuda:0")
    assert not ops.pair_cn_backward(g.rowptr, g.col, c, e, e, torch.zeros(0, device="cuda:0")).any()


@pytest.mark.parametrize("f,ldx", [(1, None), (3, None), (58, None), (64, None), (128, None), (384, None), (1500, None),
                                   (2500, None), (61, 67), (600, 601)])
@pytest.mark.parametrize("kind", ["unit", "weighted"])
def test_features_backward_vs_fp64(eps, dev, f, ldx, kind):
    from eps_amd import ops
    n = 300
    A = random_graph(n, 1500, seed=f, weighted=(kind == "weighted"), isolated=5)
    A = ssp.csr_matrix(A + ssp.diags(np.r_[np.zeros(n - 8), np.ones(3), np.zeros(5)]))    # three self loops
    A.sort_indices()
    x_dev, x_np = features(n, f, seed=f + 1, ldx=ldx)
    r0 = 10                                     # x'_r0 exactly zero although r0 has neighbours: it and they carry zero features
    assert A.indptr[r0 + 1] > A.indptr[r0]
    zero_rows = np.r_[r0, A.indices[A.indptr[r0]:A.indptr[r0 + 1]]]
    x_np[zero_rows] = 0.0
    x_dev[torch.from_numpy(zero_rows).cuda()] = 0.0
    g, revpos, xhat, nrm, _ = forward_pieces(eps, A, x_dev)
    assert float(nrm[r0]) == np.float32(1e-8) and not xhat[r0].any()
    gc_np = np.random.default_rng(f).standard_normal(A.nnz).astype(np.float32)
    gc = torch.from_numpy(gc_np).cuda()
    gxp, gxs = ops.cos_features_backward(g.rowptr, g.col, g.val, xhat, nrm, revpos, gc, want_scaled=True)
    only = ops.cos_features_backward(g.rowptr, g.col, g.val, xhat, nrm, revpos, gc)
    assert torch.equal(only, gxp)
    assert gxp.stride(0) % 32 == 0 and gxp.data_ptr() % 128 == 0
    pad = gxp.as_strided((n, gxp.stride(0)), (gxp.stride(0), 1))[:, f:]
    assert not pad.any(), "pad columns of gxp are zero"
    got, got_s = gxp.cpu().numpy(), gxs.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(got_s).all(), "the backward must be finite (clamped row included)"
    row = np.repeat(np.arange(n), np.diff(A.indptr))
    Gd = np.zeros((n, n))
    Gd[row, A.indices] = gc_np
    t = cosine_grad_truth(A, x_np.astype(np.float64), np.zeros((2, 0), np.int64), np.zeros(0), gc_given=Gd)
    truth, mag = t["gxp"]
    tol = grad_tolerance(mag, f, 1.0)
    assert worst(f"feature backward {kind} F={f} ldx={ldx}", got, truth, tol) <= 1.0
    deg = np.asarray(A.sum(1)).ravel() + 1e-6
    assert worst("  ... scaled by 1/deg", got_s, truth / deg[:, None], tol / deg[:, None]) <= 1.0
    assert np.abs(got[r0]).max() > 1.0, "the clamped row's gradient is a / 1e-8"


def _model(n, f_in, hidden, model_type="mlpcos"):
    from eps_amd import models
    emb = torch.nn.Embedding(n, hidden).cuda()
    return models.CommonNeighborsPredictor(emb, hidden + f_in, hidden, hidden, 3, 0.0, model_type=model_type).cuda()


def reference_loss(out, n_pos):
    """train_and_eval.py:73-75."""
    return -torch.log(out[:n_pos] + 1e-8).mean() - torch.log(1 - out[n_pos:] + 1e-8).mean()


def loss_gradient_truth(A, xin, pairs, n_pos):
    """(float64 loss, dL/draw per pair) of the reference's loss at the float64 raw scores."""
    raw = torch.tensor(cosine_grad_truth(A, xin, pairs, np.zeros(pairs.shape[1]))["raw"][0], requires_grad=True)
    loss = reference_loss(torch.sigmoid(raw), n_pos)
    loss.backward()
    return float(loss.detach()), raw.grad.numpy()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("with_x", [True, False])
def test_model_gradient_vs_fp64(eps, dev, weighted, with_x):
    n, hidden, f_in = 500, 32, 128
    A = random_graph(n, 4000, seed=11, weighted=weighted, isolated=3)
    g = device_graph(eps, A)
    x_dev, x_np = features(n, f_in, seed=2)
    model = _model(n, f_in if with_x else 0, hidden).train()
    n_pos = 2000
    pairs = np.concatenate([special_pairs(n, n_pos - 40 - 500, 5), all_pairs_sample(n, 2000, 6)], 1)
    n_pos = pairs.shape[1] - 2000
    out = model(x_dev if with_x else None, torch.from_numpy(pairs), g)
    assert out.requires_grad and out.shape == (pairs.shape[1],)
    loss = reference_loss(out, n_pos)
    loss.backward()
    w = model.emb.weight
    assert all(p.grad is None for p in model.mlp.parameters()), "the MLP is never applied: its parameters take no gradient"
    xin = w.detach().cpu().numpy().astype(np.float64)
    if with_x:
        xin = np.concatenate([xin, x_np.astype(np.float64)], 1)
    loss64, g_raw = loss_gradient_truth(A, xin, pairs, n_pos)
    assert abs(float(loss) - loss64) <= 1e-4
    t = cosine_grad_truth(A, xin, pairs, g_raw)
    truth, mag = t["gx"][0][:, :hidden], t["gx"][1][:, :hidden]
    got = w.grad.cpu().numpy()
    assert got.shape == truth.shape and np.isfinite(got).all()
    tol = grad_tolerance(mag, xin.shape[1], np.abs(g_raw).max())
    assert worst(f"emb.weight.grad weighted={weighted} x={with_x}", got, truth, tol) <= 1.0
    assert np.abs(truth).max() > 0


def test_five_adam_steps_follow_a_float64_replica(eps, dev):
    """Fixed batches, the same initial embedding, Adam at the reference's ddi learning rate: the float32 GPU model and a dense
    float64 torch replica.  Bound: an embedding entry after k steps is emb0 plus k Adam updates of size <= lr, so its sum of
    |terms| is |emb0| + k lr; the bar 1e-5 (4 + F/64) is taken relative to that (+ the 1e-3 floor), times k because the error
    of a step feeds the forward of the next."""
    n, hidden, steps, lr = 400, 32, 5, 0.005
    A = random_graph(n, 3000, seed=4, isolated=2)
    g = device_graph(eps, A)
    torch.manual_seed(3)
    model = _model(n, 0, hidden).train()
    emb0 = model.emb.weight.detach().cpu().numpy().astype(np.float64)
    ref = torch.tensor(emb0, requires_grad=True)
    opt = torch.optim.Adam([p for p in model.parameters()], lr=lr)
    opt64 = torch.optim.Adam([ref], lr=lr)
    Ad = A.toarray()
    losses, losses64 = [], []
    for k in range(steps):
        pairs = np.concatenate([all_pairs_sample(n, 1500, 100 + k), all_pairs_sample(n, 1500, 200 + k)], 1)
        opt.zero_grad()
        loss = reference_loss(model(None, torch.from_numpy(pairs), g), 1500)
        loss.backward()
        opt.step()
        opt64.zero_grad()
        loss64 = reference_loss(torch.sigmoid(literal_raw_dense(Ad, ref, pairs)), 1500)
        loss64.backward()
        opt64.step()
        losses.append(float(loss)), losses64.append(float(loss64))
    # the loss on ONE fixed batch before and after
    pairs = np.concatenate([all_pairs_sample(n, 1500, 100), all_pairs_sample(n, 1500, 200)], 1)
    with torch.no_grad():
        after = float(reference_loss(model(None, torch.from_numpy(pairs), g), 1500))
        after64 = float(reference_loss(torch.sigmoid(literal_raw_dense(Ad, ref, pairs)), 1500))
    print(f"[cosine-train] losses {losses} -> {after}; float64 {losses64} -> {after64}")
    assert after < losses[0] and after64 < losses64[0], "the loss on the first batch falls"
    got = model.emb.weight.detach().cpu().numpy()
    tol = steps * 1e-5 * (4 + hidden / 64) * (np.abs(emb0) + steps * lr + 1e-3)
    assert worst("embedding after 5 Adam steps", got, ref.detach().numpy(), tol) <= 1.0


def test_scoring_is_untouched_and_memory_does_not_grow(eps, dev):
    from eps_amd import heuristics
    n, hidden, f_in = 500, 32, 64
    A = random_graph(n, 4000, seed=12, weighted=True)
    g = device_graph(eps, A)
    x_dev, _ = features(n, f_in, seed=5)
    model = _model(n, f_in, hidden)
    edges = torch.from_numpy(all_pairs_sample(n, 3000, 1))
    opt = torch.optim.Adam(model.parameters(), lr=0.005)

    def scores_match():
        model.eval()
        with torch.no_grad():
            s = model(x_dev, edges, g)
        assert not s.requires_grad
        want = heuristics.cosine_common_neighbors(g, torch.cat([model.emb.weight.detach(), x_dev], 1), edges)
        assert torch.equal(s, want)
        model.eval()
        assert not model(x_dev, edges, g).requires_grad, "eval mode scores without an autograd graph"
        return s

    before = scores_match()
    mem = {}
    for step in range(1, 21):
        model.train()
        opt.zero_grad()
        loss = reference_loss(model(x_dev, edges, g), 1500)
        loss.backward()
        opt.step()
        del loss
        torch.cuda.synchronize()
        mem[step] = torch.cuda.memory_allocated()
        if step == 1:
            assert not torch.equal(scores_match(), before), "a training step changes the scores"
            mem[1] = torch.cuda.memory_allocated()
    print(f"[cosine-train] memory_allocated after step 3: {mem[3]}, after step 20: {mem[20]}")
    assert mem[20] <= mem[3]
    scores_match()


def test_non_symmetric_adjacency_is_refused(eps, dev, monkeypatch):
    from eps_amd import heuristics, ops
    from test_gpu_cosine_cn import directed_graph
    g = device_graph(eps, directed_graph(200, 1500, seed=1))

    def boom(*a, **k):
        raise AssertionError("a kernel of the cosine path was launched")

    monkeypatch.setattr(ops, "cos_node_features", boom)
    monkeypatch.setattr(ops, "pair_cn_backward", boom)
    x = torch.randn(200, 16, device="cuda:0", requires_grad=True)
    with pytest.raises(eps.EpsError, match="symmetric"):
        heuristics.cosine_common_neighbors_raw(g, x, torch.from_numpy(all_pairs_sample(200, 100, 1)))


def test_rank_cli_trains_mlpcos_and_filter_loads_checkpoint(eps, tmp_path, monkeypatch, capsys):
    """rank.py --model mlpcos --train_cosine on the collab stand-in: finite losses, a checkpoint with the reference's keys, and
    filter.py scores candidates with it."""
    import json
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.02")
    from eps_amd import filter_stage, rank_stage, training
    losses = []
    orig = training.train

    def spy(*a, **k):
        losses.append(orig(*a, **k))
        return losses[-1]

    monkeypatch.setattr(rank_stage, "train", spy)
    torch.manual_seed(1)
    curves = rank_stage.main(["--dataset", "collab", "--model", "mlpcos", "--synthetic", "--train_cosine", "--epochs", "2",
                              "--runs", "1", "--save_models"])
    assert len(losses) == 2 and all(np.isfinite(l) and l > 0 for l in losses), losses
    assert "Loss: " in capsys.readouterr().out
    assert len(curves) == 1
    ckpts = os.listdir("models")
    assert ckpts == ["collab_mlpcos||0|0.pt"], ckpts
    state = torch.load(os.path.join("models", ckpts[0]))
    keys = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["MLP_L3"]
    assert sorted(state.keys()) == sorted(["mlp." + k for k in keys] + ["emb.weight"])
    assert bool(torch.isfinite(state["emb.weight"]).all())
    fname = filter_stage.main(["--dataset", "collab", "--model", "mlpcos", "--checkpoint", ckpts[0], "--synthetic",
                               "--keep_top", "1000"])
    got = torch.load(fname)
    assert got.shape == (1000, 3) and bool((got[:-1, 2] >= got[1:, 2]).all()) and 0.0 < float(got[0, 2]) <= 1.0
