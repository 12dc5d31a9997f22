"""CPU: the float64 truth of the gradient of the cosine common-neighbour score ('mlpcos' / 'simplecos' training,
train_and_eval.py:31-96 through models.py:528-575) that the GPU tests check against, the new ABI symbols, and the CLI flag.

The truth is a closed form in numpy float64 (``cosine_grad_truth``) that also carries, for every gradient component, the sum of
the ABSOLUTE values of its terms -- every product of the restatement replaced by the product of absolute values -- which is
what the float32 tolerance is relative to.  It is checked here against torch autograd of a literal dense float64 forward."""
import argparse
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as ssp
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from test_cosine_cn_host import all_pairs_sample, random_graph


# ---------------------------------------------------------------------------------------------------------- restatement
def cosine_grad_truth(A, x, pairs, g, gc_given=None):
    """Float64 gradients of L = sum_p g[p] * raw_p (raw_p: models.py:566-574 before the sigmoid) on a SYMMETRIC adjacency.
    -> dict of (value, magnitude) pairs, dense:
         'raw' [E], 'c' [n, n] (the edge cosines on A's pattern), 'gc' [n, n] (dL/dc per stored entry), 'gxp' [n, F]
         (dL/dx'), 'gx' [n, F] (dL/dx), and 'nrm' [n], 'xhat' [n, F] without magnitudes.
    Closed form: xhat = smoothed unit features; C = mask * (xhat xhat^T); raw = (C C^T)[u, v];
    gc = mask * ((P + P^T) C) with P[u, v] = sum of g over the pairs (u, v); a = (gc + gc^T) xhat;
    gxp = (a - xhat (xhat . a)) / nrm, or a / 1e-8 where the clamp is active; gx = gxp + A^T (gxp / deg).
    ``gc_given`` (dense [n, n]) replaces the gc of the pairs: the feature backward alone, for an arbitrary dL/dc."""
    A = ssp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    Ad, Aabs = A.toarray(), abs(A).toarray()
    M = (ssp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape).toarray() > 0).astype(np.float64)
    x = np.asarray(x, np.float64)
    g = np.asarray(g, np.float64)
    u, v = np.asarray(pairs[0]), np.asarray(pairs[1])
    deg = Ad.sum(1) + 1e-6
    xp = x + (Ad @ x) / deg[:, None]
    xp_mag = np.abs(x) + (Aabs @ np.abs(x)) / np.abs(deg)[:, None]
    nrm = np.maximum(np.linalg.norm(xp, axis=1), 1e-8)
    clamped = np.linalg.norm(xp, axis=1) <= 1e-8
    xhat, xhat_mag = xp / nrm[:, None], xp_mag / nrm[:, None]
    C, Cm = M * (xhat @ xhat.T), M * (xhat_mag @ xhat_mag.T)
    raw, raw_mag = (C @ C.T)[u, v], (Cm @ Cm.T)[u, v]
    P, Pm = np.zeros((n, n)), np.zeros((n, n))
    np.add.at(P, (u, v), g)
    np.add.at(Pm, (u, v), np.abs(g))
    gc, gc_mag = M * ((P + P.T) @ C), M * ((Pm + Pm.T) @ Cm)
    if gc_given is not None:
        gc, gc_mag = M * np.asarray(gc_given, np.float64), M * np.abs(np.asarray(gc_given, np.float64))
    a, a_mag = (gc + gc.T) @ xhat, (gc_mag + gc_mag.T) @ xhat_mag
    proj = (xhat * a).sum(1, keepdims=True)
    proj_mag = (xhat_mag * a_mag).sum(1, keepdims=True)
    gxp = np.where(clamped[:, None], a / 1e-8, (a - xhat * proj) / nrm[:, None])
    gxp_mag = np.where(clamped[:, None], a_mag / 1e-8, (a_mag + xhat_mag * proj_mag) / nrm[:, None])
    gx = gxp + Ad.T @ (gxp / deg[:, None])
    gx_mag = gxp_mag + Aabs.T @ (gxp_mag / np.abs(deg)[:, None])
    return {"raw": (raw, raw_mag), "c": (C, Cm), "gc": (gc, gc_mag), "gxp": (gxp, gxp_mag), "gx": (gx, gx_mag),
            "nrm": nrm, "xhat": xhat, "mask": M}


def grad_tolerance(mag, f: int, g_scale: float):
    """The project's parity bar for float32 kernels in the form of score_tolerance / check_prologue: 1e-5 * (4 + F/64) relative
    to the sum of |terms| of the component, plus an absolute floor of 1e-3 of the incoming gradient's scale at the same
    factor (a component whose terms all vanish still sees the rounding of its neighbours' cosines)."""
    return 1e-5 * (4.0 + f / 64.0) * (np.asarray(mag) + 1e-3 * g_scale)


def literal_raw_dense(A: np.ndarray, x: torch.Tensor, pairs: np.ndarray) -> torch.Tensor:
    """The raw scores of CommonNeighborsPredictor.forward (models.py:528-574) transcribed literally in dense float64 torch with
    ``x`` a leaf: the sparse product adj[u] * adj[v], its indices, the degrees, the smoothing, two F.cosine_similarity per
    (pair, common neighbour) and the per-pair sum (test_cosine_cn_host.reference_forward_dense without the sigmoid)."""
    adj = torch.tensor(A, dtype=torch.float64)
    e = torch.tensor(pairs, dtype=torch.long)
    common = (adj[e[0]] * adj[e[1]]).to_sparse().coalesce()           # :536
    idx = common.indices()                                            # :544
    degrees = adj.sum(-1) + 1e-6                                      # :547
    left = idx.clone()
    left[0] = e[0][idx[0]]                                            # :557-558
    right = idx.clone()
    right[0] = e[1][idx[0]]                                           # :560-561
    xs = x + (adj @ x) / degrees.unsqueeze(1)                         # :562
    lf, rf = xs[left], xs[right]
    lw = F.cosine_similarity(lf[0], lf[1], dim=1)                     # :567
    rw = F.cosine_similarity(rf[0], rf[1], dim=1)                     # :568
    return torch.zeros(e.shape[1], dtype=torch.float64).index_add_(0, idx[0], lw * rw)   # :570-574


def small_case(f, weighted, seed=0):
    """The small graph of test_cosine_cn_host with a self loop added: isolated nodes, a zero feature row with neighbours, a zero
    row that stays zero, pairs with u == v, duplicated pairs and pairs without a common neighbour."""
    n = 60
    A = random_graph(n, 150, seed=3 + f + seed, weighted=weighted, isolated=4)
    A = ssp.csr_matrix(A + ssp.diags(np.r_[np.zeros(7), 2.0 if weighted else 1.0, np.zeros(n - 8)]))   # a self loop at node 7
    A.sort_indices()
    rng = np.random.default_rng(f + seed)
    x = rng.standard_normal((n, f))
    x[5] = 0.0
    x[n - 1] = 0.0
    pairs = np.concatenate([all_pairs_sample(n, 400, 7 + seed),
                            np.array([[n - 1, n - 2, 0, 5, 7, 7, 3, 3], [0, n - 1, n - 3, 5, 7, 9, 11, 11]])], 1)
    g = rng.standard_normal(pairs.shape[1])
    return A, x, pairs, g


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("f", [1, 3, 17])
def test_closed_form_gradient_equals_autograd_of_the_literal_forward(weighted, f):
    A, x, pairs, g = small_case(f, weighted)
    t = cosine_grad_truth(A, x, pairs, g)
    xl = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    raw = literal_raw_dense(A.toarray(), xl, pairs)
    np.testing.assert_allclose(t["raw"][0], raw.detach().numpy(), rtol=0, atol=1e-12)
    (raw * torch.tensor(g)).sum().backward()
    got = xl.grad.numpy()
    assert np.isfinite(got).all()
    scale = t["gx"][1].max()                # (F = 1: every cosine is +-1 and the true gradient is exactly zero)
    assert scale > 0 and (f == 1 or np.abs(got).max() > 1e-3 * scale)
    np.testing.assert_allclose(t["gx"][0], got, rtol=0, atol=1e-11 * scale)
    # the magnitudes bound the values, term by term
    for key in ("raw", "gc", "gxp", "gx"):
        assert np.all(np.abs(t[key][0]) <= t[key][1] * (1 + 1e-12) + 1e-300), key
    # pairs without a common neighbour add nothing: with only those pairs the gradient is zero
    lonely = np.array([[A.shape[0] - 1, A.shape[0] - 2], [0, A.shape[0] - 1]])
    z = cosine_grad_truth(A, x, lonely, np.ones(2))
    assert not z["gc"][0].any() and not z["gx"][0].any()


def test_closed_form_clamped_row_with_neighbours_is_finite():
    """A row whose smoothed x' is exactly zero although it has neighbours (its own feature cancels the neighbours' mean):
    the clamp is active, the gradient is a / 1e-8, finite, and autograd agrees."""
    n, f = 6, 4
    A = ssp.csr_matrix(np.array([[0, 1, 1, 0, 0, 0], [1, 0, 1, 1, 0, 0], [1, 1, 0, 0, 1, 0], [0, 1, 0, 0, 1, 0],
                                 [0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=np.float64))
    x = np.random.default_rng(1).standard_normal((n, f))
    x[1:3] = 0.0
    x[0] = 0.0                                                       # node 0: neighbours 1, 2 are zero rows -> x'_0 = 0
    pairs = np.array([[1, 0, 3, 0], [2, 3, 4, 0]])
    g = np.array([0.5, -1.0, 2.0, 0.25])
    t = cosine_grad_truth(A, x, pairs, g)
    assert t["nrm"][0] == 1e-8 and not t["xhat"][0].any()
    assert np.isfinite(t["gx"][0]).all()
    xl = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (literal_raw_dense(A.toarray(), xl, pairs) * torch.tensor(g)).sum().backward()
    got = xl.grad.numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(t["gx"][0], got, rtol=0, atol=1e-9 * max(1.0, np.abs(got).max()))


NEW_SYMBOLS = ["eps_cos_node_features_nrm", "eps_pair_cn_backward_workspace_bytes", "eps_pair_cn_backward",
               "eps_cos_features_backward"]


def test_new_abi_symbols_and_argument_checks(eps):
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "eps_abi.h")).read()
    lib = eps.load()
    for s in NEW_SYMBOLS:
        assert s + "(" in header, f"{s} not declared"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in eps._lib.SIGNATURES
    assert lib.eps_version() == 7
    assert lib.eps_pair_cn_backward_workspace_bytes(100) >= 800
    # EINVAL before any HIP call: checkable without a GPU
    rc = lib.eps_cos_node_features_nrm(None, None, None, 10, None, 8, 8, None, 8, None, None)
    assert rc == -1 and b"null" in lib.eps_last_error()
    rc = lib.eps_cos_node_features_nrm(None, None, None, 10, None, 4, 8, None, 8, None, None)
    assert rc == -1 and b"bad shape" in lib.eps_last_error()
    rc = lib.eps_pair_cn_backward(None, None, None, 10, 20, None, None, None, 5, None, None, 0, None)
    assert rc == -1 and b"null" in lib.eps_last_error()
    rc = lib.eps_pair_cn_backward(None, None, None, 10, -1, None, None, None, 5, None, None, 0, None)
    assert rc == -1 and b"negative" in lib.eps_last_error()
    rc = lib.eps_pair_cn_backward(None, None, None, 1 << 31, 20, None, None, None, 5, None, None, 0, None)
    assert rc == -1 and b"int32" in lib.eps_last_error()
    rc = lib.eps_cos_features_backward(None, None, None, 10, None, 8, 8, None, None, None, None, None, 8, None)
    assert rc == -1 and b"null" in lib.eps_last_error()
    rc = lib.eps_cos_features_backward(None, None, None, 10, None, 8, 9, None, None, None, None, None, 12, None)
    assert rc == -1 and b"bad shape" in lib.eps_last_error()
    rc = lib.eps_cos_features_backward(None, None, None, 1 << 31, None, 8, 8, None, None, None, None, None, 8, None)
    assert rc == -1


def test_new_ops_refuse_cpu_tensors(eps):
    from eps_amd import heuristics, ops
    rp, col = torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32)
    one = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(eps.EpsError):
        ops.pair_cn_backward(rp, col, torch.zeros(2), one, one, torch.zeros(1))
    with pytest.raises(eps.EpsError):
        ops.cos_features_backward(rp, col, None, torch.zeros(2, 4), torch.ones(2), col, torch.zeros(2))
    with pytest.raises(eps.EpsError):
        ops.cos_node_features(rp, col, None, torch.zeros(2, 4), want_norm=True)
    g = eps.add_edges("ddi", torch.tensor([[0, 1], [1, 2]]), torch.ones(2), torch.zeros(2, 0, dtype=torch.long), 3)
    with pytest.raises(eps.EpsError):
        heuristics.cosine_common_neighbors_raw(g, torch.zeros(3, 4, requires_grad=True), torch.tensor([[0], [2]]))


def test_parser_accepts_train_cosine_and_the_refusal_names_it(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from eps_amd import rank_stage
    args = rank_stage.make_parser().parse_args(["--dataset", "collab", "--model", "mlpcos", "--synthetic", "--train_cosine"])
    assert args.train_cosine is True
    assert rank_stage.make_parser().parse_args(["--dataset", "collab"]).train_cosine is False
    with pytest.raises(NotImplementedError, match="--train_cosine"):
        rank_stage.main(["--dataset", "collab", "--model", "mlpcos", "--synthetic", "--runs", "1"])
    assert not os.path.exists(tmp_path / "models") and not os.path.exists(tmp_path / "curves")


def test_mlpcos_model_keeps_the_golden_keys_and_a_trainable_embedding():
    from eps_amd.models import build_model
    a = argparse.Namespace(model="mlpcos", dataset="collab", num_layers=3, hidden_channels=16, dropout=0.0,
                           use_feature=True, use_learnable_embedding=True)
    model = build_model(a, SimpleNamespace(num_nodes=10, x=torch.zeros(10, 4)), "cpu")
    keys = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["MLP_L3"]
    assert sorted(model.state_dict().keys()) == sorted(["mlp." + k for k in keys] + ["emb.weight"])
    assert model.emb.weight.requires_grad
