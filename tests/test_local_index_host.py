"""CPU: the degree-normalised local indices (salton, jaccard, sorensen, hpi, hdi, lhn, pa) -- the truth helper against a brute-force
set intersection, the model factory and its defaults, the ABI table, and every argument check of csrc/local_index.hip (they
return before any HIP call)."""
import argparse
import ctypes

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import local_index_truth as lit

NAMES = ("salton", "jaccard", "sorensen", "hpi", "hdi", "lhn", "pa")


def _twelve_node_graph():
    """12 nodes: a hub (0), a triangle, a path, a pendant pair, one isolated node (11); symmetric, weighted (the values must not
    matter)."""
    e = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (2, 3), (3, 6), (6, 7), (7, 8), (4, 8), (9, 10), (5, 9), (1, 8)]
    r = np.array([a for a, b in e] + [b for a, b in e])
    c = np.array([b for a, b in e] + [a for a, b in e])
    w = np.random.default_rng(3).integers(2, 9, len(e)).astype(np.float64)
    return ssp.csr_matrix((np.r_[w, w], (r, c)), shape=(12, 12))


def test_truth_helper_against_set_intersection():
    A = _twelve_node_graph()
    nbr = [set(A.indices[A.indptr[i]:A.indptr[i + 1]]) for i in range(12)]
    assert len(nbr[11]) == 0
    u, v = (x.ravel() for x in np.meshgrid(np.arange(12), np.arange(12), indexing="ij"))      # every pair: edges, u == v, isolated
    c = lit.common_counts(A, u, v)
    assert [int(x) for x in c] == [len(nbr[a] & nbr[b]) for a, b in zip(u, v)]
    assert [int(x) for x in lit.degrees(A)] == [len(s) for s in nbr]
    for name in NAMES:
        got = lit.truth(A, u, v, name)
        assert got.dtype == np.float32
        for i, (a, b) in enumerate(zip(u, v)):
            cc, ka, kb = len(nbr[a] & nbr[b]), len(nbr[a]), len(nbr[b])
            num, den = {"salton": (cc, (ka * kb) ** 0.5), "jaccard": (cc, ka + kb - cc), "sorensen": (2 * cc, ka + kb),
                        "hpi": (cc, min(ka, kb)), "hdi": (cc, max(ka, kb)), "lhn": (cc, ka * kb), "pa": (ka * kb, 1)}[name]
            want = np.float32(num / den) if den else np.float32(0.0)
            assert got[i] == want, (name, a, b)
        assert np.array_equal(got.reshape(12, 12), got.reshape(12, 12).T), name               # score(u, v) == score(v, u)
        assert np.all(got.reshape(12, 12)[11] == 0.0)                                          # an isolated node scores 0
    cu, cv, cc = lit.two_hop_candidates(A)
    want = sorted((b, a) for a in range(12) for b in range(12) if a != b and b not in nbr[a] and nbr[a] & nbr[b])
    assert sorted(zip(cv.tolist(), cu.tolist())) == want and list(zip(cv.tolist(), cu.tolist())) == want   # column-major
    assert np.array_equal(cc, lit.common_counts(A, cu, cv))


def _args(dataset, model):
    return argparse.Namespace(dataset=dataset, model=model, num_layers=None, hidden_channels=None, dropout=None, batch_size=None,
                              lr=None, epochs=None, use_feature=None, use_learnable_embedding=None)


@pytest.mark.parametrize("name", NAMES)
def test_factory_and_defaults(eps, name):
    from eps_amd import heuristics, models, ops
    assert heuristics.LOCAL_INDICES == NAMES and tuple(ops.LOCAL_INDEX) == NAMES
    assert [ops.LOCAL_INDEX[n] for n in NAMES] == list(range(7))
    for dataset in ("collab", "ddi", "ppa"):
        args = models.default_model_configs(_args(dataset, name))
        assert args.use_feature is False and args.use_learnable_embedding is False
        simple = models.default_model_configs(_args(dataset, "simple"))
        assert vars(args) == dict(vars(simple), model=name)                                    # treated like 'simple'
        data = argparse.Namespace(num_nodes=12, x=torch.zeros(12, 4))
        m = models.build_model(args, data, "cpu")
        assert isinstance(m, models.CommonNeighborsPredictor) and m.type == name
        assert sum(p.numel() for p in m.parameters()) == 0
    with pytest.raises(AssertionError):
        models.build_model(_args("ddi", "jaccard2"), argparse.Namespace(num_nodes=12, x=None), "cpu")


def test_filter_stage_routes_the_names_past_the_scan(eps):
    from eps_amd import filter_stage
    for name in NAMES:
        assert filter_stage.fused_node_weights(argparse.Namespace(model=name), None, None) is None
        with pytest.raises(ValueError, match="no MLP decode"):
            filter_stage.check_decode_args(argparse.Namespace(model=name, decode_precision="bf16", decode_guard=None, keep_top=10))


def test_signatures_hold_the_three_entries(eps):
    sig = eps._lib.SIGNATURES
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert sig["eps_local_index_pairs"] == (ctypes.c_int, [vp, i64, vp, vp, vp, i64, i32, vp, vp])
    assert sig["eps_local_index_columns_workspace_bytes"] == (i64, [i64])
    assert sig["eps_local_index_columns"] == (ctypes.c_int, [vp, i64, i64, i64, vp, vp, vp, i64, vp, vp, i32, vp, vp, i64, vp, vp,
                                                            vp, vp, i64, vp])
    lib = eps.load()
    assert lib.eps_version() == 7
    # one int64 per slice of 4096 slots, and the total
    assert [lib.eps_local_index_columns_workspace_bytes(n) for n in (-5, 0, 1, 4096, 4097)] == [0, 0, 16, 16, 24]


def _columns(lib, **over):
    """eps_local_index_columns with arguments that pass every check but the one overridden (fake non-null pointers: a refused
    call touches none of them)."""
    p = ctypes.c_void_p(4096)
    a = dict(rowptr=p, n_nodes=100, v_lo=0, v_hi=10, colptr=p, counts=None, cand_u=p, n_slots=50, cn_i=p, cn_f=None, index=1,
             score=p, bar=None, capacity=0, surv_pos=None, surv_score=None, n_surv=None, ws=None, ws_bytes=0)
    a.update(over)
    rc = lib.eps_local_index_columns(a["rowptr"], a["n_nodes"], a["v_lo"], a["v_hi"], a["colptr"], a["counts"], a["cand_u"],
                                     a["n_slots"], a["cn_i"], a["cn_f"], a["index"], a["score"], a["bar"], a["capacity"],
                                     a["surv_pos"], a["surv_score"], a["n_surv"], a["ws"], a["ws_bytes"], None)
    return rc, lib.eps_last_error().decode()


def test_einval_without_a_gpu(eps):
    lib = eps.load()
    p = ctypes.c_void_p(4096)
    for bad in (-1, 7, 1 << 20):
        rc, msg = _columns(lib, index=bad)
        assert rc == -1 and f"index={bad}" in msg
        rc = lib.eps_local_index_pairs(p, 100, p, p, p, 5, bad, p, None)
        assert rc == -1 and f"index={bad}" in lib.eps_last_error().decode()
    rc, msg = _columns(lib, cn_f=p)
    assert rc == -1 and "both" in msg
    rc, msg = _columns(lib, cn_i=None)
    assert rc == -1 and "neither" in msg
    rc, msg = _columns(lib, v_lo=11)
    assert rc == -1 and "v_lo=11" in msg and "v_hi=10" in msg
    rc, msg = _columns(lib, v_hi=101)
    assert rc == -1 and "v_hi=101" in msg
    for key, shown in (("n_nodes", "n_nodes"), ("n_slots", "n_slots"), ("capacity", "capacity"), ("ws_bytes", "workspace_bytes")):
        rc, msg = _columns(lib, **{key: -3})
        assert rc == -1 and f"{shown}=-3" in msg, msg
    rc = lib.eps_local_index_pairs(p, 100, p, p, p, -2, 0, p, None)
    assert rc == -1 and "n_pairs=-2" in lib.eps_last_error().decode()
    rc = lib.eps_local_index_pairs(p, -1, p, p, p, 2, 0, p, None)
    assert rc == -1 and "n_nodes=-1" in lib.eps_last_error().decode()
    # a bar without a survivor list
    rc, msg = _columns(lib, bar=p, capacity=8, surv_pos=p, surv_score=p, n_surv=None, ws=p, ws_bytes=64)
    assert rc == -1 and "survivor list" in msg
    rc, msg = _columns(lib, bar=p, capacity=8, surv_pos=None, surv_score=p, n_surv=p, ws=p, ws_bytes=64)
    assert rc == -1 and "survivor list" in msg and "capacity=8" in msg
    # ... and with one, a workspace too small
    rc, msg = _columns(lib, bar=p, capacity=8, surv_pos=p, surv_score=p, n_surv=p, ws=p, ws_bytes=8)
    assert rc == -1 and "workspace" in msg and "=16" in msg
    # the float count form is exact below 2^24 nodes only
    rc, msg = _columns(lib, cn_i=None, cn_f=p, n_nodes=1 << 24, v_hi=10)
    assert rc == -1 and f"n_nodes={1 << 24}" in msg and "2^24" in msg
    rc, msg = _columns(lib, score=None)
    assert rc == -1 and "nothing to compute" in msg
    rc, msg = _columns(lib, v_lo=10, v_hi=10)
    assert rc == -1 and "empty block" in msg
    # nothing to do is not an error (and launches nothing)
    assert lib.eps_local_index_pairs(None, 0, None, None, None, 0, 3, None, None) == 0
    assert _columns(lib, n_slots=0, v_lo=10, v_hi=10, rowptr=None, colptr=None, cand_u=None, score=None)[0] == 0


def test_ops_refuse_what_the_kernel_must_not_see(eps):
    from eps_amd import ops
    z32, z64 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(eps.EpsError):                       # CPU tensors: no fallback
        ops.local_index_pairs(z64, 3, z32, z32, z32, "jaccard")
    with pytest.raises(eps.EpsError):
        ops.local_index_columns(z64, 3, 0, 3, z64, z32, z32, "jaccard")
    with pytest.raises(eps.EpsError, match="one of salton"):
        ops._local_index_code("cosine")
