"""CPU: the truths of tests/cn_list_truth.py against a brute-force dense statement, the ABI surface of the common-neighbour
list unit (csrc/pair_cn_list.hip), and the NCN models' factory, state-dict keys, defaults, refusals and decoder formula."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import cn_list_truth as ct
from conftest import ROOT

KEYS = ["num_layers", "hidden_channels", "dropout", "batch_size", "lr", "epochs", "use_feature", "use_learnable_embedding"]
SYMBOLS = ["eps_pair_cn_list_limits", "eps_pair_cn_list_count", "eps_pair_cn_list_fill", "eps_cn_list_transpose_workspace_bytes",
           "eps_cn_list_transpose"]


def _small_graphs():
    rng = np.random.default_rng(2)
    dense = (rng.random((40, 40)) < 0.3)
    dense = dense | dense.T                                                    # symmetric, with self loops
    sparse_dir = rng.random((60, 60)) < 0.06                                   # directed, several empty rows
    sparse_dir[::7] = False
    star = np.zeros((30, 30), bool)
    star[0, 1:] = star[1:, 0] = True                                           # a hub: every pair of leaves shares exactly it
    star[5, 6] = star[6, 5] = True
    return [dense, sparse_dir, star]


@pytest.mark.parametrize("gi", [0, 1, 2])
def test_truths_agree_with_the_dense_statement(gi):
    D = _small_graphs()[gi]
    n = D.shape[0]
    A = ssp.csr_matrix(D.astype(np.float32) * 2.5)                             # (values are not ones: only the pattern counts)
    rng = np.random.default_rng(3)
    u = np.concatenate([rng.integers(0, n, 200), np.arange(n), [-1, n, 0]])
    v = np.concatenate([rng.integers(0, n, 200), np.arange(n), [0, 0, n + 5]])
    ptr, w = ct.cn_lists(A, u, v)
    assert ptr[0] == 0 and ptr[-1] == len(w) and len(ptr) == len(u) + 1
    for b, (a, c) in enumerate(zip(u, v)):
        want = np.flatnonzero(D[a] & D[c]) if 0 <= a < n and 0 <= c < n else np.zeros(0, np.int64)
        assert w[ptr[b]:ptr[b + 1]].tolist() == want.tolist(), (b, a, c)
    assert ptr[-3:].tolist() == [len(w)] * 3                                   # the three pairs with an id outside the graph
    # the transpose: node -> the pairs that list it, ascending
    tptr, tb = ct.transpose_stable(ptr, w, n)
    C = ct.incidence(ptr, w, n).toarray() > 0
    assert tptr[0] == 0 and tptr[-1] == len(w)
    for node in range(n):
        assert tb[tptr[node]:tptr[node + 1]].tolist() == np.flatnonzero(C[:, node]).tolist()
    # the sums: sequential float32 adds in list order, and float64
    h = rng.standard_normal((n, 5)).astype(np.float32)
    z32 = ct.seq_sum_f32(ptr, w, h)
    z64, zabs = ct.sum_f64(ptr, w, h, n)
    for b in range(len(u)):
        acc = np.zeros(5, np.float32)
        for node in w[ptr[b]:ptr[b + 1]]:
            acc = acc + h[node]
        assert z32[b].tobytes() == acc.tobytes()
    np.testing.assert_allclose(z64, C.astype(np.float64) @ h.astype(np.float64), rtol=0, atol=1e-12)
    bound = ct.gamma(np.diff(ptr))[:, None] * zabs
    assert bool((np.abs(z32.astype(np.float64) - z64) <= bound).all())
    g = rng.standard_normal((len(u), 5)).astype(np.float32)
    d32 = ct.seq_sum_f32(tptr, tb, g)
    np.testing.assert_allclose(d32, C.T.astype(np.float64) @ g.astype(np.float64), rtol=0, atol=1e-4)


def test_dense_ncn_forward_restates_the_sparse_sum():
    """ncn_forward's z = (P[u] * P[v]) @ h is the incidence product of cn_lists."""
    D = _small_graphs()[0]
    n = D.shape[0]
    P = torch.from_numpy(D.astype(np.float64))
    h = torch.randn(n, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    e = torch.randint(0, n, (2, 50), generator=torch.Generator().manual_seed(2))
    ptr, w = ct.cn_lists(ssp.csr_matrix(D.astype(np.float32)), e[0].numpy(), e[1].numpy())
    z = (P[e[0]] * P[e[1]]) @ h
    np.testing.assert_allclose(z.numpy(), ct.sum_f64(ptr, w, h.numpy(), n)[0], rtol=0, atol=1e-12)


def test_boundary_graph_has_the_rows_it_promises():
    cap, ratio = 1024, 32
    A, special, stranger = ct.boundary_graph(cap, ratio)
    deg = np.diff(A.indptr)
    assert deg[special].tolist() == ct.boundary_lengths(cap, ratio) and deg[stranger] == 64
    assert (A != A.T).nnz == 0 and A.data.max() > 1
    u, v = ct.boundary_pairs(A, special, stranger)
    assert len(u) == 11 * 11 + 1000 and u.dtype == np.int32


# ---------------------------------------------------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_bound_and_exported(eps):
    text = open(os.path.join(ROOT, "include", "eps_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = eps.load()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in eps_abi.h"
        assert s in eps._lib.SIGNATURES and hasattr(lib, s)
    assert lib.eps_version() == eps._lib.ABI_VERSION == 7
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    sig = eps._lib.SIGNATURES
    assert sig["eps_pair_cn_list_count"] == (ctypes.c_int, [vp, vp, i64, vp, vp, i64, vp, vp])
    assert sig["eps_pair_cn_list_fill"] == (ctypes.c_int, [vp, vp, i64, vp, vp, i64, vp, vp, vp, vp])
    assert sig["eps_cn_list_transpose"] == (ctypes.c_int, [vp, vp, i64, i64, i64, vp, vp, vp, i64, vp])
    makefile = open(os.path.join(ROOT, "edge-proposal-sets_amd", "csrc", "Makefile")).read()
    assert "pair_cn_list.hip" in re.search(r"^SRCS\s*:?=\s*(.*)$", makefile, flags=re.M).group(1).split()


def test_host_queries_and_refusals_without_a_gpu(eps):
    from eps_amd import ops
    cap, ratio = ops.pair_cn_list_limits()
    assert cap >= 64 and cap & (cap - 1) == 0 and ratio >= 2
    lib = eps.load()
    assert lib.eps_cn_list_transpose_workspace_bytes(0, 10) == 256
    # EINVAL paths return before any HIP call
    assert lib.eps_pair_cn_list_count(None, None, -1, None, None, 5, None, None) == -1 and b"n_rows=-1" in lib.eps_last_error()
    assert lib.eps_pair_cn_list_count(None, None, 10, None, None, 5, None, None) == -1 and b"null" in lib.eps_last_error()
    assert lib.eps_pair_cn_list_count(None, None, 10, None, None, 0, None, None) == 0
    assert lib.eps_pair_cn_list_fill(None, None, 10, None, None, 5, None, None, None, None) == -1 and b"status" in lib.eps_last_error()
    assert lib.eps_cn_list_transpose(None, None, 1 << 31, 4, 4, None, None, None, 0, None) == -1 and b"m=2147483648" in lib.eps_last_error()
    assert lib.eps_cn_list_transpose(None, None, 3, 0, 4, None, None, None, 0, None) == -1
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(eps.EpsError):
        ops.pair_cn_list(torch.zeros(4, dtype=torch.int64), z, 3, z, z)        # CPU tensors: no fallback


# ---------------------------------------------------------------------------------------------------------- the models
def _args(dataset, model, **over):
    a = argparse.Namespace(dataset=dataset, model=model, **{k: None for k in KEYS})
    vars(a).update(over)
    return a


@pytest.mark.parametrize("name,encoder", [("ncn", "gcn"), ("ncn_sage", "sage")])
def test_factory_keys_and_defaults(eps, name, encoder):
    from eps_amd import models
    for dataset in ("ddi", "collab", "reddit", "email"):
        got = models.default_model_configs(_args(dataset, name))
        want = models.default_model_configs(_args(dataset, encoder))
        assert vars(got) == dict(vars(want), model=name), dataset
        assert got.hidden_channels is not None and got.num_layers >= 2
    args = models.default_model_configs(_args("collab", name, hidden_channels=16))
    data = argparse.Namespace(num_nodes=12, x=torch.zeros(12, 4))
    m = models.build_model(args, data, "cpu")
    assert type(m) is models.NCNLinkGNN and isinstance(m, models.LinkGNN) and type(m.linkpred) is models.NCNPredictor
    assert type(m.gnn) is (models.GCN if encoder == "gcn" else models.SAGE)
    assert m.emb.weight.shape == (12, 16) and m.linkpred.beta == 1.0 and not isinstance(m.linkpred.beta, torch.Tensor)
    L = args.num_layers
    assert L == 3
    conv = ([f"gnn.convs.{i}.{k}" for i in range(L) for k in ("weight", "bias")] if encoder == "gcn" else
            [f"gnn.convs.{i}.{k}" for i in range(L) for k in ("lin_l.weight", "lin_l.bias", "lin_r.weight")])
    want_keys = (["emb.weight"] + conv + [f"linkpred.{l}.{k}" for l in ("xij_lin", "xcn_lin") for k in ("weight", "bias")]
                 + [f"linkpred.lins.{i}.{k}" for i in range(L - 1) for k in ("weight", "bias")])
    assert sorted(m.state_dict()) == sorted(want_keys)
    sd = m.state_dict()
    assert sd["linkpred.xij_lin.weight"].shape == sd["linkpred.xcn_lin.weight"].shape == (16, 16)
    assert sd[f"linkpred.lins.{L - 2}.weight"].shape == (1, 16) and sd["linkpred.lins.0.weight"].shape == (16, 16)
    assert sd["gnn.convs.0." + ("weight" if encoder == "gcn" else "lin_l.weight")].numel() == (16 + 4) * 16


@pytest.mark.parametrize("name", ["ncn", "ncn_sage"])
def test_refusals_fire_before_any_data_is_touched(eps, name):
    from eps_amd import models

    class Untouchable:
        def __getattr__(self, k):
            raise AssertionError(f"build_model read data.{k} before refusing")

    args = models.default_model_configs(_args("ppa", name))                    # ppa has no defaults: no width
    assert args.hidden_channels is None
    with pytest.raises(models.UnsupportedModelConfig, match="hidden_channels"):
        models.build_model(args, Untouchable(), "cpu")
    args = models.default_model_configs(_args("ddi", name, num_layers=1))
    with pytest.raises(models.UnsupportedModelConfig, match="num_layers 1"):
        models.build_model(args, Untouchable(), "cpu")
    with pytest.raises(ValueError):
        models.NCNPredictor(8, 8, 1, 1, 0.0)


def test_parsers_and_stage_guards_take_the_names(eps, monkeypatch):
    from eps_amd import filter_stage, rank_stage
    for name in ("ncn", "ncn_sage"):
        filter_stage.check_ncn_args(argparse.Namespace(model=name))
        with monkeypatch.context() as mp:                                      # sharded filter runs are not part of the model
            mp.setenv("WORLD_SIZE", "2")
            filter_stage.check_ncn_args(argparse.Namespace(model="gcn"))
            with pytest.raises(ValueError, match="one process"):
                filter_stage.check_ncn_args(argparse.Namespace(model=name))
        assert rank_stage.make_parser().parse_args(["--dataset", "ddi", "--model", name]).model == name
        assert filter_stage.make_parser().parse_args(["--dataset", "ddi", "--model", name, "--checkpoint", "c||0|0.pt"]).model == name
        with pytest.raises(ValueError, match="no MLP decode"):
            filter_stage.check_decode_args(argparse.Namespace(model=name, decode_precision="bf16", decode_guard=None, keep_top=10))
        assert filter_stage.fused_node_weights(argparse.Namespace(model=name), None, None) is None
        for flag, msg in (("fused_decode", "--fused_decode trains"), ("fused_decode_bn", "--fused_decode_bn trains")):
            a = rank_stage.make_parser().parse_args(["--dataset", "ddi", "--model", name, "--" + flag])
            with pytest.raises(ValueError, match=msg):
                rank_stage.run(a)


@pytest.mark.parametrize("layers,beta", [(2, 1.0), (3, 0.5), (4, 2.0)])
def test_predictor_is_the_formula(eps, layers, beta):
    from eps_amd import models
    torch.manual_seed(layers)
    m = models.NCNPredictor(12, 20, 1, layers, 0.5, beta=beta).eval()
    assert len(m.lins) == layers - 1 and m.lins[-1].out_features == 1
    xi, xj, z = torch.randn(37, 12), torch.randn(37, 12), 3 * torch.randn(37, 12)
    with torch.no_grad():
        got = m(xi, xj, z)
    assert got.shape == (37, 1)
    p = {k: v.double() for k, v in m.state_dict().items()}
    t = (torch.relu((xi.double() * xj.double()) @ p["xij_lin.weight"].t() + p["xij_lin.bias"])
         + beta * torch.relu(z.double() @ p["xcn_lin.weight"].t() + p["xcn_lin.bias"]))
    for i in range(layers - 2):
        t = torch.relu(t @ p[f"lins.{i}.weight"].t() + p[f"lins.{i}.bias"])
    want = torch.sigmoid(t @ p[f"lins.{layers - 2}.weight"].t() + p[f"lins.{layers - 2}.bias"])
    assert float((got.double() - want).abs().max()) <= 1e-6
    assert float((ct.ncn_predictor(xi.double() * xj.double(), z.double(), p, beta, "") - want.squeeze(1)).abs().max()) <= 1e-12
    # training mode: dropout is applied (the outputs differ from eval), and reset_parameters redraws every layer
    m.train()
    assert not torch.equal(m(xi, xj, z), got)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.reset_parameters()
    assert all(not torch.equal(before[k], v) for k, v in m.state_dict().items() if k.endswith("weight"))
