"""CPU: the float64 restatement of the cosine common-neighbour models (models.py:528-575, 'simplecos' / 'mlpcos') the GPU tests
check against, the mlpcos state-dict keys, and the raw-cut translation of a sigmoid bar used by the fused filter path."""
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


# ---------------------------------------------------------------------------------------------------------- restatement
def smoothed_unit_features(A: ssp.csr_matrix, x: np.ndarray) -> np.ndarray:
    """xhat of models.py:546-569 in float64: x' = x + (A @ x) / (rowsum(A) + 1e-6) (:547, :562; A's values), each row
    divided by max(||x'||_2, 1e-8) (F.cosine_similarity's per-vector clamp, torch 2.x)."""
    A = ssp.csr_matrix(A, dtype=np.float64)
    x = np.asarray(x, np.float64)
    deg = np.asarray(A.sum(1)).ravel() + 1e-6
    xp = x + (A @ x) / deg[:, None]
    return xp / np.maximum(np.linalg.norm(xp, axis=1), 1e-8)[:, None]


def edge_cosines_truth(A: ssp.csr_matrix, xhat: np.ndarray):
    """(c, sum of |terms|) per stored entry of A, in A's CSR order (sorted indices)."""
    A = ssp.csr_matrix(A)
    A.sort_indices()
    row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    prod = xhat[row] * xhat[A.indices]
    return prod.sum(1), np.abs(prod).sum(1)


def raw_scores_truth(A: ssp.csr_matrix, x: np.ndarray, pairs: np.ndarray):
    """(raw, sum of |terms|) of models.py:566-575 before the sigmoid: sum over w in N(u) & N(v) (the stored PATTERN of A:
    only the indices of the product are used, :544) of cos(x'_u, x'_w) * cos(x'_v, x'_w).  pairs: [2, E]."""
    A = ssp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    xhat = smoothed_unit_features(A, x)
    c, _ = edge_cosines_truth(A, xhat)
    C = ssp.csr_matrix((c, A.indices, A.indptr), shape=A.shape)
    Cabs = ssp.csr_matrix((np.abs(c), A.indices, A.indptr), shape=A.shape)
    u, v = np.asarray(pairs[0]), np.asarray(pairs[1])
    if u.size > 50_000 and A.shape[0] <= 5000:          # whole candidate sets of small stand-ins: C C^T densely
        Cd, Cad = C.toarray(), Cabs.toarray()
        return (Cd @ Cd.T)[u, v], (Cad @ Cad.T)[u, v]
    raw = np.asarray(C[u].multiply(C[v]).sum(1)).ravel()
    mag = np.asarray(Cabs[u].multiply(Cabs[v]).sum(1)).ravel()
    return raw, mag


def scores_truth(A, x, pairs):
    raw, mag = raw_scores_truth(A, x, pairs)
    return 1.0 / (1.0 + np.exp(-raw)), mag


def score_tolerance(mag, f: int):
    """Float32 accumulation in the kernels: relative to sum |terms| (not to the sum), a sigmoid's slope is <= 1/4."""
    return 1e-5 * (4.0 + f / 64.0) * (1.0 + mag) + 1e-6


def reference_forward_dense(A: np.ndarray, x: np.ndarray, pairs: np.ndarray) -> np.ndarray:
    """A literal dense transcription of CommonNeighborsPredictor.forward (models.py:528-575) for simplecos, in float64 torch:
    the sparse product adj[u] * adj[v], its indices, the degrees, the smoothing, two F.cosine_similarity calls per
    (pair, common neighbour), the per-pair sum and the sigmoid."""
    adj = torch.tensor(A, dtype=torch.float64)
    x = torch.tensor(x, dtype=torch.float64)
    e = torch.tensor(pairs, dtype=torch.long)
    common = (adj[e[0]] * adj[e[1]]).to_sparse().coalesce()           # :536
    idx = common.indices()                                            # :544
    degrees = adj.sum(-1) + 1e-6                                      # :547
    left = idx.clone()
    left[0] = e[0][idx[0]]                                            # :557-558
    right = idx.clone()
    right[0] = e[1][idx[0]]                                           # :560-561
    x = x + (adj @ x) / degrees.unsqueeze(1)                          # :562
    lf, rf = x[left], x[right]
    lw = F.cosine_similarity(lf[0], lf[1], dim=1)                     # :567
    rw = F.cosine_similarity(rf[0], rf[1], dim=1)                     # :568
    out = torch.zeros(e.shape[1], dtype=torch.float64).index_add_(0, idx[0], lw * rw)   # :570-574
    return torch.sigmoid(out).numpy()                                 # :575


def random_graph(n, m, seed, weighted=False, isolated=0):
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n - isolated, m), rng.integers(0, n - isolated, m)
    keep = r != c
    r, c = r[keep], c[keep]
    w = rng.integers(1, 6, r.size).astype(np.float64) if weighted else np.ones(r.size)
    A = ssp.coo_matrix((np.concatenate([w, w]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def all_pairs_sample(n, k, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n, k), rng.integers(0, n, k)])


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("f", [1, 3, 17])
def test_restatement_equals_the_literal_forward(weighted, f):
    n = 60
    A = random_graph(n, 150, seed=3 + f, weighted=weighted, isolated=4)     # the last 4 nodes have no edge
    rng = np.random.default_rng(f)
    x = rng.standard_normal((n, f))
    x[5] = 0.0                                                              # a zero feature row (smoothed by its neighbours)
    x[n - 1] = 0.0                                                          # a zero row that stays zero: isolated
    pairs = np.concatenate([all_pairs_sample(n, 400, 7),
                            np.array([[n - 1, n - 2, 0, 5], [0, n - 1, n - 3, 5]])], 1)   # isolated ends: no common neighbour
    got, _ = scores_truth(A, x, pairs)
    ref = reference_forward_dense(A.toarray(), x, pairs)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    assert np.all(got[-4:-1] == 0.5), "pairs without a common neighbour score sigmoid(0) = 0.5"
    assert np.any(got != 0.5)


def test_restatement_on_a_golden_graph():
    d = np.load(os.path.join(GOLDEN, "pairs_star50.npz"))
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((d["val"].astype(np.float64), d["col"], d["rowptr"]), shape=(n, n))
    x = np.random.default_rng(0).standard_normal((n, 5))
    got, _ = scores_truth(A, x, d["pairs"])
    np.testing.assert_allclose(got, reference_forward_dense(A.toarray(), x, d["pairs"]), rtol=0, atol=1e-12)


def _args(model, **kw):
    a = argparse.Namespace(model=model, dataset="collab", num_layers=3, hidden_channels=16, dropout=0.0,
                           use_feature=True, use_learnable_embedding=True)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_mlpcos_state_dict_keys():
    from eps_amd.models import build_model
    data = SimpleNamespace(num_nodes=10, x=torch.zeros(10, 4))
    model = build_model(_args("mlpcos"), data, "cpu")
    keys = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["MLP_L3"]
    assert sorted(model.state_dict().keys()) == sorted(["mlp." + k for k in keys] + ["emb.weight"])
    assert model.mlp.lins[0].in_features == 16 + 4 and model.mlp.lins[-1].out_features == 16
    simple = build_model(_args("simplecos", use_learnable_embedding=False), data, "cpu")
    assert list(simple.state_dict().keys()) == []


def test_cosine_models_need_features():
    from eps_amd.models import build_model
    with pytest.raises(ValueError, match="no node features"):
        build_model(_args("simplecos", use_learnable_embedding=False), SimpleNamespace(num_nodes=10, x=None), "cpu")
    with pytest.raises(ValueError, match="needs node features"):
        build_model(_args("simplecos", use_feature=None, use_learnable_embedding=False),
                    SimpleNamespace(num_nodes=10, x=torch.zeros(10, 2)), "cpu")


def test_rank_mlpcos_fails_before_any_work(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from eps_amd import rank_stage
    with pytest.raises(NotImplementedError, match="mlpcos"):
        rank_stage.main(["--dataset", "collab", "--model", "mlpcos", "--synthetic", "--runs", "1"])
    assert not os.path.exists(tmp_path / "models") or not os.listdir(tmp_path / "models")


def _bars():
    rng = np.random.default_rng(0)
    one = np.float32(1.0)
    near_one = [np.nextafter(one, np.float32(0))]
    for _ in range(300):
        near_one.append(np.nextafter(near_one[-1], np.float32(0)))
    half = [np.float32(0.5)]
    for d in (1, -1):
        b = np.float32(0.5)
        for _ in range(100):
            b = np.nextafter(b, np.float32(d))
            half.append(b)
    dense = np.linspace(0.0, 1.0, 2001, dtype=np.float32)
    sig = torch.sigmoid(torch.tensor(rng.uniform(-30, 30, 3000), dtype=torch.float32)).numpy()
    return np.unique(np.concatenate([near_one, half, dense, sig, [one, np.float32(1e-30), np.float32(0.0)]]).astype(np.float32))


def test_raw_cut_is_conservative():
    """For every bar b: no float32 raw value r <= t = sigmoid_raw_cut(b) has torch.sigmoid(r) > b (CPU float32), checked on
    the 64 float32 values at and below t and on a coarse sweep further down; and t is not loose by more than a few ulps of
    the score."""
    from eps_amd.heuristics import sigmoid_raw_cut
    bars = _bars()
    ts = np.array([sigmoid_raw_cut(float(b)) for b in bars], dtype=np.float64)
    assert np.isinf(ts[bars == np.float32(1.0)]).all() and (ts[bars == np.float32(1.0)] > 0).all()
    fin = np.isfinite(ts)
    t32 = ts[fin].astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), ts[fin]), "the threshold is a float32 value"
    steps = [t32]
    for _ in range(63):
        steps.append(np.nextafter(steps[-1], np.float32(-np.inf)))
    coarse = [t32 - np.float32(d) for d in (0.01, 0.1, 1.0, 10.0)]
    r = np.stack(steps + coarse, 1)
    s = torch.sigmoid(torch.from_numpy(r)).numpy()
    assert (s <= bars[fin][:, None]).all(), "a raw value at or below the cut has a sigmoid above the bar"
    # ... and the cut is tight: the value 4 score-ulps above the bar's logit passes it
    b = bars[fin].astype(np.float64)
    inner = (b > 1e-3) & (b < 1 - 2 ** -20)
    lo = np.log(b[inner] + 8 * 2.0 ** -24) - np.log1p(-(b[inner] + 8 * 2.0 ** -24))
    assert (ts[fin][inner] < lo).all()
    assert (ts[fin][inner] > np.log(b[inner] - 8 * 2.0 ** -24) - np.log1p(-(b[inner] - 8 * 2.0 ** -24)) - 1e-6).all()
