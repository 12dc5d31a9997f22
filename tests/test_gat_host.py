"""CPU: the graph-attention truth (tests/gat_truth.py) against literal formulations, its case builders against what they promise,
its forward bound against a careful float32 evaluation, the model factory's handling of --model gat, and the argument validation
of eps_gat_aggregate (EINVAL paths return before any HIP call)."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import gat_truth as gt

KEYS = ["num_layers", "hidden_channels", "dropout", "batch_size", "lr", "epochs", "use_feature", "use_learnable_embedding"]
CONV_KEYS = ("lin.weight", "att_src", "att_dst", "bias")


# ------------------------------------------------------------------------------------------------------------- the truth
def _small(seed=3, n=40, f=8, heads=2):
    """A small symmetric graph with an empty row, a loop-only row and a loop among others, and random operands (float64)."""
    rng = np.random.default_rng(seed)
    M = rng.random((n, n)) < 0.15
    M = np.triu(M, 1)
    M = M | M.T
    M[0, :] = M[:, 0] = False                     # an empty row
    M[1, :] = M[:, 1] = False
    M[1, 1] = True                                # only a stored self loop
    M[2, 2] = True                                # a stored self loop among others
    import scipy.sparse as ssp
    A = ssp.csr_matrix(M.astype(np.float64))
    A.sort_indices()
    z = rng.standard_normal((n, f))
    return A, z, rng.standard_normal((n, heads)), rng.standard_normal((n, heads)), rng.standard_normal(f), rng.standard_normal((n, f))


def test_forward_truth_is_the_triple_loop_and_the_dense_softmax():
    A, z, ss, sd, bias, _ = _small()
    n, f, heads = A.shape[0], z.shape[1], ss.shape[1]
    C = f // heads
    got = gt.aggregate(A.indptr, A.indices, z, ss, sd, heads, bias)
    want = np.zeros((n, f))
    for i in range(n):
        nb = sorted({int(c) for c in A.indices[A.indptr[i]:A.indptr[i + 1]]} | {i})     # the self loop exactly once
        for h in range(heads):
            e = []
            for j in nb:
                raw = ss[j, h] + sd[i, h]
                e.append(raw if raw > 0 else 0.2 * raw)
            den = sum(np.exp(v) for v in e)
            for c in range(C):
                want[i, h * C + c] = sum(np.exp(v) / den * z[j, h * C + c] for v, j in zip(e, nb)) + bias[h * C + c]
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[0], z[0] + bias) and np.array_equal(got[1], z[1] + bias)      # an empty row, a loop-only row: z[i] + bias
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    dense = gt.dense_aggregate(gt.dense_mask(A), t(z), t(ss), t(sd), heads) + t(bias)
    assert float((dense - t(got)).abs().max()) <= 1e-12
    assert np.array_equal(gt.aggregate(A.indptr, A.indices, z, ss, sd, heads, bias, relu=True), np.maximum(got, 0))
    # a row block with row0 gives those rows
    blk = gt.aggregate(A.indptr[2:6], A.indices, z, ss, sd, heads, bias, row0=2)
    assert np.array_equal(blk, got[2:5])
    parts = gt.aggregate(A.indptr, A.indices, z, ss, sd, heads, parts=True)
    raw = t(ss)[None, :, :] + t(sd)[:, None, :]
    e = torch.nn.functional.leaky_relu(raw, 0.2).masked_fill(~gt.dense_mask(A)[:, :, None], float("-inf"))
    assert float((torch.logsumexp(e, 1) - t(parts["lse"])).abs().max()) <= 1e-12


def test_backward_truth_is_autograd_through_the_dense_formulation():
    A, z, ss, sd, _, gout = _small(seed=4)
    heads = ss.shape[1]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)
    zt, st, dt = t(z), t(ss), t(sd)
    out = gt.dense_aggregate(gt.dense_mask(A), zt, st, dt, heads)
    out.backward(torch.from_numpy(gout))
    got = gt.aggregate_backward(A.indptr, A.indices, z, ss, sd, heads, out.detach().numpy(), gout)
    for name, want in (("gz", zt.grad), ("g_s_src", st.grad), ("g_s_dst", dt.grad)):
        assert np.abs(got[name] - want.numpy()).max() <= 1e-11, name
        assert (got[name + "_bound"] >= 0).all() and np.isfinite(got[name + "_bound"]).all()


def test_conv_and_model_truths_follow_the_published_layer():
    """gat_conv is the aggregate truth on z = x W^T and the two inner products; link_gnn_forward chains it."""
    A, _, _, _, _, _ = _small(seed=6, f=8)
    rng = np.random.default_rng(0)
    n, heads, C, fin = A.shape[0], 2, 4, 6
    p = {"lin.weight": rng.standard_normal((heads * C, fin)), "att_src": rng.standard_normal((1, heads, C)),
         "att_dst": rng.standard_normal((1, heads, C)), "bias": rng.standard_normal(heads * C)}
    x = rng.standard_normal((n, fin))
    z = x @ p["lin.weight"].T
    z3 = z.reshape(n, heads, C)
    want = gt.aggregate(A.indptr, A.indices, z, (z3 * p["att_src"]).sum(-1), (z3 * p["att_dst"]).sum(-1), heads, p["bias"], relu=True)
    got = gt.gat_conv({k: torch.from_numpy(v) for k, v in p.items()}, gt.dense_mask(A), torch.from_numpy(x), heads, relu=True)
    assert np.abs(got.numpy() - want).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------ the builders
def test_graph_holds_what_it_promises():
    A = gt.graph()
    assert A.shape == (gt.N_NODES, gt.N_NODES) and (A != A.T).nnz == 0 and A.has_sorted_indices
    deg = np.diff(A.indptr)
    row = lambda i: A.indices[A.indptr[i]:A.indptr[i + 1]].tolist()
    assert deg[:len(gt.ROW_LENGTHS)].tolist() == gt.ROW_LENGTHS
    for want in (0, 1, 2, 31, 32, 33, 63, 64, 65, 300):
        assert want in deg[:len(gt.ROW_LENGTHS)]
    assert deg[gt.EMPTY_ROW] == 0 and deg[gt.CHUNK_ROW] == 64 and deg[gt.HUB_ROW] == 300 > 4 * 64
    assert row(gt.LOOP_ONLY_ROW) == [gt.LOOP_ONLY_ROW]
    assert gt.LOOP_ROW in row(gt.LOOP_ROW) and len(row(gt.LOOP_ROW)) == gt.LOOP_ROW_OTHERS + 1
    assert A.diagonal().nonzero()[0].tolist() == [gt.LOOP_ONLY_ROW, gt.LOOP_ROW]
    assert all(min(row(i)) > i for i in range(1, 10))                       # own id sorts before all its neighbours
    last = gt.N_NODES - 1
    assert row(last) and max(row(last)) < last                             # ... after all of them
    mid = gt.between_row(A)
    assert min(row(mid)) < mid < max(row(mid)) and mid not in row(mid)     # ... in between
    B = gt.asymmetric(A)
    assert (B != B.T).nnz > 0 and B.nnz < A.nnz


@pytest.mark.parametrize("f,heads", gt.SHAPES)
def test_regimes_hold_what_they_promise(f, heads):
    assert f % (4 * heads) == 0
    c = gt.case(f, heads, "quarters")
    A = c["A"]
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    for i, j in ((rows, A.indices), (np.arange(A.shape[0]), np.arange(A.shape[0]))):
        raw = c["s_src"][j].astype(np.float64) + c["s_dst"][i].astype(np.float64)
        assert np.abs(raw).min() >= 1 / 16 and np.array_equal(np.round(raw * 8) % 2, np.ones_like(raw))      # odd multiples of 1/8
    c = gt.case(f, heads, "wide")
    args = gt.exp_arguments(c["rowptr"], c["col"], c["s_src"], c["s_dst"])
    raw = c["s_src"][A.indices].astype(np.float32) + c["s_dst"][rows].astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(raw.astype(np.float32))).any()                                                # a naive float32 exp overflows
    assert raw.max() == 90.0 and raw.min() < -60.0 and args.max() == 0.0
    tr = gt.forward_truth(f, heads, "wide", True, False)
    assert np.isfinite(tr["out"]).all() and np.isfinite(tr["lse"]).all()                                      # ... the truth stays finite
    J = gt.neighbourhood(c["rowptr"], c["col"], gt.EQUAL_ROW, gt.EQUAL_ROW)
    e = c["s_src"][J] + c["s_dst"][gt.EQUAL_ROW][None, :]
    assert len(J) == 32 and (e == e[0]).all()                                                                # one row's scores all equal
    want = c["z"][J].astype(np.float64).mean(0) + c["bias"]
    assert np.abs(tr["out"][gt.EQUAL_ROW] - want).max() <= 1e-12


def test_exp_ulps_is_twice_the_measured_worst():
    worst = 0.0
    for f, heads in gt.SHAPES:
        for regime in gt.REGIMES:
            c = gt.case(f, heads, regime)
            worst = max(worst, gt.worst_exp_ulps(gt.exp_arguments(c["rowptr"], c["col"], c["s_src"], c["s_dst"])))
    print(f"worst float32 exp error on the cases' arguments: {worst:.3f} ulp; EXP_ULPS = {gt.EXP_ULPS}")
    assert 0.0 < 2.0 * worst <= gt.EXP_ULPS <= 2.0 * worst + 0.1 + 1e-9


@pytest.mark.parametrize("regime", gt.REGIMES)
@pytest.mark.parametrize("f,heads", gt.SHAPES)
def test_careful_float32_stays_inside_the_forward_bound(f, heads, regime):
    """The bound is neither vacuous nor too tight: a max-subtracted float32 numpy evaluation keeps inside it, and uses a visible
    part of it."""
    c = gt.case(f, heads, regime)
    tr = gt.forward_truth(f, heads, regime, True, True)
    got = gt.aggregate_float32(c["rowptr"], c["col"], c["z"], c["s_src"], c["s_dst"], heads, c["bias"], relu=True)
    ratio = np.abs(got - tr["out"]) / np.maximum(tr["bound"], 1e-300)
    print(f"f={f} heads={heads} {regime}: float32 numpy error / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0 and ratio.max() >= 0.01
    assert (tr["bound"][gt.HUB_ROW] > 0).all() and tr["bound"].max() < 1e-2


# -------------------------------------------------------------------------------------------------------------- the factory
def _args(dataset, model, **over):
    a = argparse.Namespace(dataset=dataset, model=model, **{k: None for k in KEYS})
    vars(a).update(over)
    return a


def test_factory_builds_gat_with_the_published_keys(eps):
    from eps_amd import models
    assert "gat" in models._MODELS
    for dataset in ("ddi", "collab", "reddit", "email"):
        got = models.default_model_configs(_args(dataset, "gat"))
        want = models.default_model_configs(_args(dataset, "gcn"))
        assert vars(got) == dict(vars(want), model="gat"), dataset
    args = models.default_model_configs(_args("collab", "gat", hidden_channels=32, gat_heads=2))
    m = models.build_model(args, argparse.Namespace(num_nodes=12, x=torch.zeros(12, 4)), "cpu")
    assert type(m) is models.LinkGNN and type(m.gnn) is models.GAT and type(m.linkpred) is models.LinkPredictor
    L = args.num_layers
    assert L == 3 and len(m.gnn.convs) == L and all(type(c) is models.GATConv and c.heads == 2 for c in m.gnn.convs)
    want_keys = (["emb.weight"] + [f"gnn.convs.{i}.{k}" for i in range(L) for k in CONV_KEYS]
                 + [f"linkpred.lins.{i}.{k}" for i in range(L) for k in ("weight", "bias")])
    assert sorted(m.state_dict()) == sorted(want_keys)
    sd = m.state_dict()
    assert sd["gnn.convs.0.lin.weight"].shape == (32, 32 + 4) and sd["gnn.convs.1.lin.weight"].shape == (32, 32)
    assert sd["gnn.convs.0.att_src"].shape == sd["gnn.convs.2.att_dst"].shape == (1, 2, 16) and sd["gnn.convs.0.bias"].shape == (32,)
    assert float(sd["gnn.convs.0.bias"].abs().max()) == 0.0 and float(sd["gnn.convs.0.att_src"].abs().max()) > 0.0
    assert hasattr(m.gnn, "forward_sharded")
    # the default head count
    m4 = models.build_model(models.default_model_configs(_args("ddi", "gat")), argparse.Namespace(num_nodes=12, x=None), "cpu")
    assert m4.gnn.convs[0].heads == 4 and m4.gnn.convs[0].att_src.shape == (1, 4, 64)


def test_factory_refuses_by_rule(eps):
    from eps_amd import models

    class Untouchable:
        def __getattr__(self, k):
            raise AssertionError(f"build_model read data.{k} before refusing")

    def refused(match, dataset="ddi", **over):
        with pytest.raises(models.UnsupportedModelConfig, match=match):
            models.build_model(models.default_model_configs(_args(dataset, "gat", **over)), Untouchable(), "cpu")

    refused("needs --hidden_channels", dataset="ppa")                        # ppa has no defaults: no width
    refused(r"not a multiple of 4 \* heads = 16.*--gat_heads 1 or 3 or 5", dataset="email")       # H = 300 with the default 4 heads
    refused(r"not a multiple of 4 \* heads = 12", hidden_channels=64, gat_heads=3)
    refused("up to 256", hidden_channels=512)
    refused("num_layers 1", num_layers=1)
    refused("--gat_heads 0", gat_heads=0)
    refused("--gat_heads 9", gat_heads=9)
    with pytest.raises(ValueError):
        models.GATConv(8, 10, heads=4)
    for name in ("sage2", "ensemble_gcn_sage"):                              # ... and the old refusal keeps its wording
        a = _args("ddi", name, hidden_channels=16, num_layers=2, dropout=0.0, use_feature=False, use_learnable_embedding=False)
        with pytest.raises(NotImplementedError, match=r"\(sage2 / ensemble_gcn_sage\) is outside the accelerated path"):
            models.build_model(a, argparse.Namespace(num_nodes=12, x=None), "cpu")


def test_parsers_and_stage_guards_take_gat(eps):
    from eps_amd import filter_stage, rank_stage
    r = rank_stage.make_parser().parse_args(["--dataset", "ddi", "--model", "gat"])
    assert r.model == "gat" and r.gat_heads is None
    assert rank_stage.make_parser().parse_args(["--dataset", "ddi", "--model", "gat", "--gat_heads", "8"]).gat_heads == 8
    f = filter_stage.make_parser().parse_args(["--dataset", "ddi", "--model", "gat", "--checkpoint", "c||0|0.pt", "--gat_heads", "2"])
    assert f.model == "gat" and f.gat_heads == 2
    assert "gat" in filter_stage.BF16_FILTER_MODELS
    ok = dict(model="gat", decode_precision="bf16", decode_guard=None, keep_top=10, hidden_channels=64)
    filter_stage.check_decode_args(argparse.Namespace(num_layers=2, **ok))
    with pytest.raises(ValueError, match="one-layer decoder"):
        filter_stage.check_decode_args(argparse.Namespace(num_layers=1, **ok))
    filter_stage.check_ncn_args(argparse.Namespace(model="gat"))            # a LinkGNN: sharded filter runs included


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_argument_validation_without_gpu(eps):
    lib = eps.load()
    cf = ctypes.c_float(0.2)

    def fwd(heads, f, n_rows=4, ptr=None):
        return lib.eps_gat_aggregate(ptr, ptr, 0, n_rows, 8, ptr, f, heads, f, ptr, ptr, max(heads, 1), cf, None, 0, ptr, f, None, None)

    for heads, f, word in ((0, 8, b"heads = 0"), (9, 72, b"heads = 9"), (2, 6, b"multiple of 4"), (3, 8, b"heads = 3 times"),
                           (4, 8, b"heads = 4 times")):                     # heads = 4, f = 8: C = 2 is no whole float4
        assert fwd(heads, f) == -1 and word in lib.eps_last_error(), (heads, f, lib.eps_last_error())
    assert fwd(2, 8) == -1 and b"null pointer" in lib.eps_last_error()
    assert fwd(2, 8, n_rows=0) == 0                                          # nothing to do: no pointer is read
    assert fwd(2, 8, n_rows=9) == -1 and b"bad shape" in lib.eps_last_error()        # the block leaves the graph
    rc = lib.eps_gat_aggregate_backward(None, None, 8, None, 8, 0, 8, None, None, 1, cf, None, None, 8, None, 8, None, 8, None, None,
                                        None, None)
    assert rc == -1 and b"heads = 0" in lib.eps_last_error()
    rc = lib.eps_gat_aggregate_backward(None, None, 8, None, 8, 2, 8, None, None, 2, cf, None, None, 8, None, 8, None, 8, None, None,
                                        None, None)
    assert rc == -1 and b"null pointer" in lib.eps_last_error()
    z = torch.zeros((3, 8))
    with pytest.raises(eps.EpsError):                                        # CPU tensors: no fallback
        eps.ops.gat_aggregate(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), z, z[:, :2], z[:, :2], 2)
