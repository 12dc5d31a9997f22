"""CPU: the local-community indices (car, cpa, caa, cra, cjc) -- names and codes, the ABI entries, the factory's defaults, the
refusals of ops.* that need no GPU, and the truth helper (tests/local_community_truth.py) against its own per-pair restatement
and against the closed forms of a clique."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import local_community_truth as lct
from conftest import GOLDEN, ROOT

NAMES = ("car", "cpa", "caa", "cra", "cjc")


def _args(dataset, model):
    return argparse.Namespace(dataset=dataset, model=model, num_layers=None, hidden_channels=None, dropout=None, batch_size=None,
                              lr=None, epochs=None, use_feature=None, use_learnable_embedding=None)


def test_names_and_codes(eps):
    from eps_amd import heuristics, ops
    assert heuristics.LOCAL_COMMUNITY_INDICES == NAMES and tuple(ops.LOCAL_COMMUNITY_INDEX) == NAMES == lct.INDICES
    assert [ops.LOCAL_COMMUNITY_INDEX[n] for n in NAMES] == list(range(5))
    assert not set(NAMES) & set(heuristics.LOCAL_INDICES) and len(heuristics.LOCAL_INDICES) == 7
    with pytest.raises(eps.EpsError, match="one of car"):
        ops._local_community_code("cn")
    with pytest.raises(eps.EpsError, match="one of car"):
        heuristics.local_community(None, None, "jaccard")


def test_signatures_in_header_and_table(eps):
    sig = eps._lib.SIGNATURES
    vp, i64, i32, pi32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)
    assert sig["eps_local_community_limits"] == (ctypes.c_int, [pi32, pi32, pi32])
    assert sig["eps_local_community_degrees"] == (ctypes.c_int, [vp, vp, i64, vp, vp, i64, vp, vp, vp])
    assert sig["eps_local_community_scores"] == (ctypes.c_int, [vp, i64, vp, vp, vp, vp, vp, i64, i32, vp, vp])
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eps_abi.h")).read(), flags=re.S)
    for name in ("eps_local_community_limits", "eps_local_community_degrees", "eps_local_community_scores"):
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    lib = eps.load()
    assert lib.eps_version() == 7
    from eps_amd import ops
    short, cap, ratio = ops.local_community_limits()
    assert 2 <= short < 64 and cap >= 64 and cap & (cap - 1) == 0 and ratio >= 2


def test_einval_without_a_gpu(eps):
    lib = eps.load()
    p = ctypes.c_void_p(4096)
    for bad in (-1, 5, 1 << 20):
        rc = lib.eps_local_community_scores(p, 100, p, p, p, p, p, 5, bad, p, None)
        assert rc == -1 and f"index={bad}" in lib.eps_last_error().decode()
    rc = lib.eps_local_community_scores(p, 100, p, p, p, p, None, 5, 0, p, None)
    assert rc == -1 and "come together" in lib.eps_last_error().decode()
    rc = lib.eps_local_community_scores(p, 100, p, p, p, p, p, -2, 0, p, None)
    assert rc == -1 and "n_pairs=-2" in lib.eps_last_error().decode()
    rc = lib.eps_local_community_degrees(p, p, 1 << 31, p, p, 5, p, p, None)
    assert rc == -1 and "bad size" in lib.eps_last_error().decode()
    rc = lib.eps_local_community_degrees(p, p, 100, p, p, 5, p, None, None)
    assert rc == -1 and "null status" in lib.eps_last_error().decode()
    assert lib.eps_local_community_scores(None, 0, None, None, None, None, None, 0, 3, None, None) == 0


@pytest.mark.parametrize("name", NAMES)
def test_factory_and_defaults(eps, name):
    from eps_amd import filter_stage, models
    for dataset in ("ddi", "collab", "ppa"):
        args = models.default_model_configs(_args(dataset, name))
        assert args.use_feature is False and args.use_learnable_embedding is False
        jac = models.default_model_configs(_args(dataset, "jaccard"))
        assert vars(args) == dict(vars(jac), model=name)
        m = models.build_model(args, argparse.Namespace(num_nodes=12, x=torch.zeros(12, 4)), "cpu")
        assert isinstance(m, models.CommonNeighborsPredictor) and m.type == name
        assert sum(p.numel() for p in m.parameters()) == 0
    assert name in models._MODELS and name in models._HEURISTICS
    assert filter_stage.fused_node_weights(argparse.Namespace(model=name), None, None) is None       # never the threshold scan
    assert name in filter_stage.LOCAL_COMMUNITY_INDICES


def test_ops_refuse_what_the_kernel_must_not_see(eps):
    from eps_amd import ops
    z32, z64 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    ptr = torch.tensor([0, 2, 4], dtype=torch.int64)
    with pytest.raises(eps.EpsError, match="CPU tensor"):           # right in every other respect: no fallback
        ops.local_community_degrees(z64, z32, 3, ptr, z32)
    with pytest.raises(eps.EpsError, match="CPU tensor"):
        ops.local_community_scores(z64, 3, z32[:2], z32[:2], ptr, z32, z32, "cra")
    with pytest.raises(eps.EpsError, match="w: expected torch.int32"):
        ops.local_community_degrees(z64, z32, 3, ptr, z64)
    with pytest.raises(eps.EpsError, match="ptr: expected torch.int64"):
        ops.local_community_degrees(z64, z32, 3, ptr.int(), z32)
    with pytest.raises(eps.EpsError, match="gamma: expected torch.int32"):
        ops.local_community_scores(z64, 3, z32[:2], z32[:2], ptr, z32, z64, "cra")
    with pytest.raises(eps.EpsError, match="rowptr must hold"):
        ops.local_community_degrees(z64, z32, 7, ptr, z32)
    with pytest.raises(eps.EpsError, match="ptr must hold 3 entries"):
        ops.local_community_scores(z64, 3, z32[:2], z32[:2], ptr[:2], z32, z32, "cra")
    with pytest.raises(eps.EpsError, match="gamma holds 3 entries, not 4"):
        ops.local_community_scores(z64, 3, z32[:2], z32[:2], ptr, z32, z32[:3], "cra")
    with pytest.raises(eps.EpsError, match="come together"):
        ops.local_community_scores(z64, 3, z32[:2], z32[:2], ptr, z32, None, "cra")
    with pytest.raises(eps.EpsError, match="one of car"):
        ops.local_community_scores(z64, 3, z32[:2], z32[:2], ptr, z32, z32, "salton")


def _golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = len(d["rowptr"]) - 1
    return ssp.csr_matrix((np.ones(len(d["col"])), d["col"], d["rowptr"]), shape=(n, n)), d["pairs"]


def test_truth_agrees_with_its_per_pair_restatement():
    A, pairs = _golden("pairs_er500")
    import local_index_truth as lit
    cu, cv, cc = lit.two_hop_candidates(A)
    pick = np.random.default_rng(0).choice(len(cu), 1500, replace=False)
    u = np.concatenate([cu[pick], pairs[0][:500]])
    v = np.concatenate([cv[pick], pairs[1][:500]])
    ptr, w, gamma = lct.pair_truth(A, u, v)
    assert np.array_equal(np.diff(ptr)[:1500], cc[pick]) and gamma.max() > 0
    assert np.array_equal(gamma, lct.gammas_by_pair(A, ptr, w))
    for index in NAMES:
        got, want = lct.scores(A, u, v, ptr, w, gamma, index), lct.scores_by_pair(A, u, v, index)
        lit.assert_within_one_ulp(got, want, index)
        assert got.max() > 0
    # an asymmetric pattern with self loops: "z stored in row w", not "w stored in row z"
    rng = np.random.default_rng(1)
    B = ssp.csr_matrix((rng.random((60, 60)) < 0.3).astype(np.float64))
    B.setdiag(1.0)
    B = ssp.csr_matrix(B)
    u, v = rng.integers(0, 60, 300), rng.integers(0, 60, 300)
    ptr, w, gamma = lct.pair_truth(B, u, v)
    assert np.array_equal(gamma, lct.gammas_by_pair(B, ptr, w))
    G = np.add.reduceat(np.r_[gamma, 0], ptr[:-1]) * (np.diff(ptr) > 0)
    assert (G % 2 == 1).any()


@pytest.mark.parametrize("n", list(range(3, 13)) + [66])
def test_closed_forms_on_a_clique(n):
    """K_n: any pair has the other n - 2 nodes in common, each adjacent to the other n - 3 of them."""
    A = lct.clique(n)
    u, v = np.nonzero(np.ones((n, n)) - np.eye(n))
    ptr, w, gamma = lct.pair_truth(A, u, v)
    c, G = n - 2, (n - 2) * (n - 3)
    assert (np.diff(ptr) == c).all() and (gamma == n - 3).all()
    car = c * G / 2.0
    want = {"car": car, "cpa": (1 + car) * (1 + car), "cra": G / (n - 1.0), "caa": G / np.log2(n - 1.0), "cjc": car / n}
    for index in NAMES:
        got = lct.scores(A, u, v, ptr, w, gamma, index)
        assert np.allclose(got, np.float32(want[index]), rtol=3e-7, atol=0), index
    assert lct.scores(A, u, v, ptr, w, gamma, "cra")[0] == np.float32(G / (n - 1.0))
