"""CPU: the truth of tests/sketch_truth.py against the check values of DESIGN 4.5h, against sketches built from explicit sets and
against exact counts; the ABI surface and refusals of the sketch unit (csrc/sketch.hip); and the buddy model's factory, layer
shapes, defaults, refusals and parser flags."""
import argparse
import ctypes

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import sketch_truth as st

KEYS = ["num_layers", "hidden_channels", "dropout", "batch_size", "lr", "epochs", "use_feature", "use_learnable_embedding"]


# ---------------------------------------------------------------------------------------------------------- check values
def test_mix64_and_own_sketch_check_values():
    assert [int(x) for x in st.mix64([0, 1, 12345])] == [0xE220A8397B1DCDAF, 0x910A2DEC89025CC1, 0x22118258A9D111A0]
    hll, mh = st.own_sketch([0, 1, 12345, 6598086])
    assert [(int(np.flatnonzero(r)[0]), int(r.max()), int((r != 0).sum())) for r in hll] == [(226, 3, 1), (145, 5, 1), (34, 4, 1), (84, 29, 1)]
    assert [int(x) for x in mh[0, :3]] == [0xA3820138, 0x7BCCB532, 0x896D31FB]
    assert int(mh[1, 0]) == 0xFD59956F and int(mh[2, 0]) == 0xA79276DE
    # rank 29 is the highest below 2^24, and 6598086 the first id to reach it
    ranks = st.own_register(np.arange(1 << 24))[1]
    assert int(ranks.max()) == 29 and int(np.argmax(ranks)) == 6598086 and int(ranks.min()) >= 1
    assert list(st.bit_length32([0, 1, 2, 3, 255, 256, 0xFFFFFFFF])) == [0, 1, 2, 2, 8, 9, 32]
    h, m = st.empty_sketch()
    assert not h.any() and (m == 0xFFFFFFFF).all()


def _graphs():
    rng = np.random.default_rng(4)
    n = 37
    path = ssp.diags([np.ones(n - 1), np.ones(n - 1)], [1, -1]).tocsr()
    star = np.zeros((n, n))
    star[0, 1:] = star[1:, 0] = 1
    clique = np.ones((9, 9)) - np.eye(9)
    rnd = (rng.random((n, n)) < 0.08).astype(float)                            # directed, with self loops and empty rows
    rnd[::6] = 0
    rnd[3, 3] = 1
    return {"path": path, "star": ssp.csr_matrix(star), "clique": ssp.csr_matrix(clique), "random": ssp.csr_matrix(rnd)}


@pytest.mark.parametrize("name", ["path", "star", "clique", "random"])
def test_propagated_tables_are_the_sketches_of_the_explicit_sets(name):
    """sketch(S_k(v)) built from the explicit sets == the propagated tables: the union algebra and the keep_own convention."""
    A = _graphs()[name]
    hll, mh = st.tables(A, 2)
    sets = st.exact_sets(A, 2)
    for k in range(2):
        for v in range(A.shape[0]):
            h, m = st.sketch_of_set(sets[k][v].indices)
            assert np.array_equal(hll[k, v], h) and np.array_equal(mh[k, v], m), (name, k, v)
    # S_1 is open: a node is in its own S_1 only through a stored self loop; S_2 follows the definition
    dense = [s.toarray() for s in sets]
    P = ssp.csr_matrix(A).toarray() != 0
    assert np.array_equal(dense[0], P)
    assert np.array_equal(dense[1], P | ((P.astype(int) @ P.astype(int)) > 0))
    # one hop table is the other's prefix
    assert np.array_equal(st.tables(A, 1)[0][0], hll[0])


def test_pair_statistics_of_special_rows():
    A = _graphs()["random"]
    hll, mh = st.tables(A, 2)
    empty = int(np.flatnonzero(np.diff(A.indptr) == 0)[0])
    sets = st.exact_sets(A, 2)
    assert sets[1][empty].nnz == 0
    S, Z, M = st.pair_stats(hll, mh, [empty, 1, -1, 1], [empty, 1, 2, A.shape[0]])
    assert (S[0] == 1 << 41).all() and (Z[0] == 256).all() and (M[0] == 128).all()
    assert (M[1].diagonal() == 128).all()
    assert (S[2:] == -1).all() and (Z[2:] == -1).all() and (M[2:] == -1).all()
    assert float(st.cardinality(1 << 41, 256)) == 0.0
    assert np.array_equal(st.row_cardinality(hll)[:, empty], [0.0, 0.0])
    # statistics of (u, v) are those of (v, u) transposed
    u, v = np.arange(20), np.arange(20)[::-1]
    a, b = st.pair_stats(hll, mh, u, v), st.pair_stats(hll, mh, v, u)
    assert all(np.array_equal(x, y.transpose(0, 2, 1)) for x, y in zip(a, b))


def test_truth_accuracy_against_exact_counts():
    """The estimator itself, on the seeded skewed graph (3,000 nodes, 36,540 stored entries, largest row 1,253) and 4,000 uniform
    pairs.  Measured: Pearson r of I_11 0.9344, I_12 0.9554, I_22 0.9942 with the exact counts; mean relative error of C_1
    0.0198, of C_2 0.0337.  Each bound leaves a third of the measured error (1 - r, or the error) as margin: the estimator is
    deterministic, the margin covers the platform's log."""
    got = st.accuracy(st.skewed_graph())
    print(got)
    assert got["I11"] >= 1 - (1 - 0.9344) * 4 / 3
    assert got["I12"] >= 1 - (1 - 0.9554) * 4 / 3
    assert got["I22"] >= 1 - (1 - 0.9942) * 4 / 3
    assert got["C1"] <= 0.0198 * 4 / 3
    assert got["C2"] <= 0.0337 * 4 / 3


def test_boundary_graph_holds_every_length_class(eps):
    from eps_amd import ops
    rc, _ = ops.sketch_limits()
    A, cls = st.boundary_graph(rc)
    n = A.shape[0]
    assert n < 2000 and n % 4 and n % 64
    assert all(cls[c] for c in st.BOUNDARY_CLASSES)
    assert A[0, 0] != 0 and A.indptr[1] == rc and A.indptr[1] % rc == 0          # row 1 (2 rc + 1) begins exactly on a cut
    assert A.indptr[2] // rc == (A.indptr[2] - 1) // rc                          # row 2 begins in the piece of row 1's tail
    last = n - 1
    assert A.indptr[last] == A.indptr[last + 1] and last in A.indices
    b, e = A.indptr[st.LONGEST_ROW], A.indptr[st.LONGEST_ROW + 1]                # five pieces: a second trip of the combine loop
    assert e - b == 3 * rc + 2 and (e - 1) // rc - b // rc == 4


def test_feature_formulas_are_the_region_sizes_on_exact_counts():
    """With exact counts in place of the estimates, the five features are log1p of the sizes of the regions they are named
    after (S_2 contains S_1 by definition, so the differences are set differences and a22 is inclusion-exclusion)."""
    A = _graphs()["random"]
    n = A.shape[0]
    S1, S2 = (s.toarray() for s in st.exact_sets(A, 2))
    rng = np.random.default_rng(1)
    u, v = rng.integers(0, n, 200), rng.integers(0, n, 200)
    I = st.exact_intersections(st.exact_sets(A, 2), u, v).astype(np.float64)
    C = np.stack([S1.sum(1), S2.sum(1)]).astype(np.float64)
    got = np.expm1(st.features(I, C[:, u], C[:, v]).astype(np.float64))
    R1u, R1v, R2u, R2v = S1[u], S1[v], S2[u] & ~S1[u], S2[v] & ~S1[v]
    want = np.stack([(R1u & R1v).sum(1), (R1u & R2v).sum(1) + (R2u & R1v).sum(1), (R2u & R2v).sum(1),
                     (R1u & ~S2[v]).sum(1) + (R1v & ~S2[u]).sum(1), (R2u & ~S2[v]).sum(1) + (R2v & ~S2[u]).sum(1)], 1)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6) and want.max() > 3
    got1 = np.expm1(st.features(I[:, :1, :1], C[:1, u], C[:1, v]).astype(np.float64))
    want1 = np.stack([(R1u & R1v).sum(1), (R1u & ~S1[v]).sum(1) + (R1v & ~S1[u]).sum(1)], 1)
    assert np.allclose(got1, want1, rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------- the library
def test_abi_surface_and_refusals_without_a_gpu(eps):
    from eps_amd import ops
    lib = eps.load()
    assert lib.eps_version() == eps._lib.ABI_VERSION == 7
    for s in ("eps_sketch_limits", "eps_sketch_own", "eps_sketch_propagate_workspace_bytes", "eps_sketch_propagate", "eps_sketch_pair_stats"):
        assert hasattr(lib, s) and s in eps._lib.SIGNATURES
    rc, ppw = ops.sketch_limits()
    assert rc >= 64 and ppw == 4
    assert lib.eps_sketch_propagate_workspace_bytes(0) == 256
    assert lib.eps_sketch_propagate_workspace_bytes(rc + 1) == 2 * 2 * 768 + 256
    # EINVAL paths return before any HIP call; the pointers below are never dereferenced
    buf = (ctypes.c_uint8 * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 256
    p, q, r, s = (ctypes.c_void_p(a + 1024 * i) for i in range(4))
    assert lib.eps_sketch_own(0, 1, None, q, None) == -1 and b"null" in lib.eps_last_error()
    assert lib.eps_sketch_own(0, -1, p, q, None) == -1
    assert lib.eps_sketch_own((1 << 31) - 3, 4, p, q, None) == -1 and b"2^31" in lib.eps_last_error()
    assert lib.eps_sketch_own(-1, 1, p, q, None) == -1
    assert lib.eps_sketch_own(1 << 31, 0, p, q, None) == 0                       # (nothing to write)
    assert lib.eps_sketch_pair_stats(None, q, 1, 4, p, p, 1, p, None) == -1 and b"null" in lib.eps_last_error()
    for k in (0, 3):
        assert lib.eps_sketch_pair_stats(p, q, k, 4, r, r, 1, s, None) == -1 and b"hops" in lib.eps_last_error()
    assert lib.eps_sketch_pair_stats(p, q, 2, -1, r, r, 1, s, None) == -1
    assert lib.eps_sketch_pair_stats(p, q, 2, 4, r, r, 0, s, None) == 0
    assert lib.eps_sketch_propagate(None, p, 1, 0, p, q, r, s, 0, None, 0, None) == -1 and b"null" in lib.eps_last_error()
    assert lib.eps_sketch_propagate(p, p, -1, 0, p, q, r, s, 0, None, 0, None) == -1
    assert lib.eps_sketch_propagate(p, p, 1, 0, p, q, p, s, 0, None, 0, None) == -1 and b"alias" in lib.eps_last_error()
    assert lib.eps_sketch_propagate(p, p, 1, 0, p, q, r, q, 1, None, 0, None) == -1 and b"alias" in lib.eps_last_error()
    assert lib.eps_sketch_propagate(p, p, 1, 3, p, q, r, s, 1, None, 0, None) == -1 and b"workspace" in lib.eps_last_error()
    assert lib.eps_sketch_propagate(p, p, 0, 0, p, q, r, s, 1, None, 0, None) == 0


def test_ops_refuse_cpu_tensors(eps):
    from eps_amd import ops
    h, m = torch.zeros((3, 256), dtype=torch.uint8), torch.zeros((3, 128), dtype=torch.uint32)
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(eps.EpsError):
        ops.sketch_own(0, 3, "cpu")
    with pytest.raises(eps.EpsError):
        ops.sketch_propagate(torch.zeros(4, dtype=torch.int64), z, 3, h, m, False)
    with pytest.raises(eps.EpsError):
        ops.sketch_pair_stats(h[None], m[None], 3, z, z)


# ---------------------------------------------------------------------------------------------------------- the model
def _args(dataset, model, **over):
    a = argparse.Namespace(dataset=dataset, model=model, **{k: None for k in KEYS})
    vars(a).update(over)
    return a


@pytest.mark.parametrize("hops,feats", [(1, 2), (2, 5)])
def test_buddy_factory_layers_and_defaults(eps, hops, feats):
    from eps_amd import models
    for dataset in ("ddi", "collab", "reddit", "email"):
        got = models.default_model_configs(_args(dataset, "buddy"))
        want = models.default_model_configs(_args(dataset, "gcn"))
        assert vars(got) == dict(vars(want), model="buddy"), dataset
    args = models.default_model_configs(_args("collab", "buddy", hidden_channels=16, sketch_hops=hops))
    m = models.build_model(args, argparse.Namespace(num_nodes=12, x=torch.zeros(12, 4)), "cpu")
    assert type(m) is models.BuddyLinkModel and not isinstance(m, models.LinkGNN) and isinstance(m, models._CachedEmbeddings)
    assert type(m.linkpred) is models.BuddyPredictor and m.hops == hops
    L = args.num_layers
    assert L == 3
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {"emb.weight": (12, 16), "feat_lin.weight": (16, (hops + 1) * 20), "feat_lin.bias": (16,),
            "linkpred.xij_lin.weight": (16, 16), "linkpred.xij_lin.bias": (16,),
            "linkpred.xs_lin.weight": (16, feats), "linkpred.xs_lin.bias": (16,),
            "linkpred.lins.0.weight": (16, 16), "linkpred.lins.0.bias": (16,),
            "linkpred.lins.1.weight": (1, 16), "linkpred.lins.1.bias": (1,)}
    assert sd == want
    # the decoder's formula, on the CPU
    p = m.linkpred.eval()
    xi, xj, f = torch.randn(7, 16), torch.randn(7, 16), torch.rand(7, feats)
    t = torch.relu(p.xij_lin(xi * xj)) + torch.relu(p.xs_lin(f))
    assert torch.equal(p(xi, xj, f), torch.sigmoid(p.lins[1](torch.relu(p.lins[0](t)))))
    assert torch.equal(p(xi, xj, f), p(xj, xi, f))


def test_buddy_refusals_and_parsers(eps, monkeypatch):
    from eps_amd import filter_stage, models, rank_stage

    class Untouchable:
        def __getattr__(self, k):
            raise AssertionError(f"build_model read data.{k} before refusing")

    args = models.default_model_configs(_args("ppa", "buddy"))                 # ppa has no defaults: no width
    assert args.hidden_channels is None
    with pytest.raises(models.UnsupportedModelConfig, match="hidden_channels"):
        models.build_model(args, Untouchable(), "cpu")
    with pytest.raises(models.UnsupportedModelConfig, match="num_layers 1"):
        models.build_model(models.default_model_configs(_args("ddi", "buddy", num_layers=1)), Untouchable(), "cpu")
    with pytest.raises(ValueError):
        models.BuddyPredictor(8, 8, 1, 1, 0.0)
    with pytest.raises(ValueError):
        models.BuddyLinkModel(None, 8, 8, 2, 0.0, hops=3)
    # sage2 / ensemble_gcn_sage stay refused with their wording
    with pytest.raises(NotImplementedError, match="outside the accelerated path"):
        models.build_model(models.default_model_configs(_args("ddi", "sage2")), argparse.Namespace(num_nodes=4, x=None), "cpu")
    filter_stage.check_ncn_args(argparse.Namespace(model="buddy"))
    with monkeypatch.context() as mp:
        mp.setenv("WORLD_SIZE", "2")
        filter_stage.check_ncn_args(argparse.Namespace(model="gcn"))
        with pytest.raises(ValueError, match="one process"):
            filter_stage.check_ncn_args(argparse.Namespace(model="buddy"))
    fa = filter_stage.make_parser().parse_args(["--dataset", "ddi", "--model", "buddy", "--checkpoint", "c||0|0.pt"])
    ra = rank_stage.make_parser().parse_args(["--dataset", "ddi", "--model", "buddy", "--sketch_hops", "1"])
    assert fa.model == ra.model == "buddy" and fa.sketch_hops == 2 and ra.sketch_hops == 1
    for parser, extra in ((filter_stage.make_parser(), ["--checkpoint", "c||0|0.pt"]), (rank_stage.make_parser(), [])):
        with pytest.raises(SystemExit):
            parser.parse_args(["--dataset", "ddi", "--model", "buddy", "--sketch_hops", "3", *extra])
    assert filter_stage.fused_node_weights(argparse.Namespace(model="buddy"), None, None) is None
    with pytest.raises(ValueError, match="no MLP decode"):
        filter_stage.check_decode_args(argparse.Namespace(model="buddy", decode_precision="bf16", decode_guard=None, keep_top=10))
