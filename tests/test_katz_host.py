"""CPU: the Katz scoring surface -- coefficients of the reference's truncated series, the golden fixtures against an fp64
restatement, the argument checks of the new C ABI entry points, and the size cap of the exact branch."""
import os

import numpy as np
import pytest
import scipy.sparse as ssp

from conftest import GOLDEN

LISTS = ["pos_train", "pos_valid", "neg_valid", "pos_test", "neg_test"]
GRAPH_OF = {"pos_train": "train", "pos_valid": "train", "neg_valid": "train", "pos_test": "full", "neg_test": "full"}


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def fixture_csr(d, tag):
    n = int(d["n"])
    return ssp.csr_matrix((d[f"{tag}_val"].astype(np.float64), d[f"{tag}_col"], d[f"{tag}_rowptr"]), shape=(n, n))


def truncated_truth(A, pairs, coeffs):
    """c1*A + c2*A^2 + c3*A^3 at the pairs, float64, without forming A^3: (A^2)[u,v] = A[u,:] . A[:,v] and
    (A^3)[u,v] = (A[u,:] A) . A[:,v]."""
    A = A.astype(np.float64).tocsr()
    AT = A.T.tocsr()
    u, v = pairs[:, 0], pairs[:, 1]
    out = np.zeros(len(u))
    for s in range(0, len(u), 2000):
        uu, vv = u[s:s + 2000], v[s:s + 2000]
        Ru, Cv = A[uu], AT[vv]
        a1 = np.asarray(A[uu, vv]).ravel()
        a2 = np.asarray(Ru.multiply(Cv).sum(1)).ravel()
        a3 = np.asarray((Ru @ A).multiply(Cv).sum(1)).ravel()
        out[s:s + 2000] = coeffs[0] * a1 + coeffs[1] * a2 + coeffs[2] * a3
    return out


def exact_truth(A, beta):
    n = A.shape[0]
    return np.linalg.inv(np.eye(n) - beta * A.toarray().astype(np.float64)) - np.eye(n)


def exact_tolerance(cond, H):
    """The reference forms beta*A in float32 (a relative perturbation of at most 2^-24 per entry) before its float64
    inverse: the prediction moves by at most ~cond * 2^-24 * |H|."""
    return cond * 2.0 ** -23 * max(1.0, float(np.abs(H).max()))


def test_katz_coefficients_follow_the_reference_loop(eps):
    from eps_amd.heuristics import katz_coefficients
    assert katz_coefficients(0.05, 2) == (0.05, 0.005, 0.000125)       # beta, 2 beta^2, beta^3: not the textbook beta^2
    assert katz_coefficients(0.05, 1) == (0.05, 0.0025, 0.0)
    assert katz_coefficients(0.05, 0) == (0.05, 0.0, 0.0)
    with pytest.raises(eps.EpsError):
        katz_coefficients(0.05, 3)


def test_collab_fixture_is_the_truncated_series(eps):
    """The reference's float32 SciPy loop == c1*A + c2*A^2 + c3*A^3 at the pairs (fp64), which pins the 2*beta^2 quirk."""
    from eps_amd.heuristics import katz_coefficients
    d = load_fixture("katz_collab_like.npz")
    assert str(d["dataset"]) == "collab"
    coeffs = katz_coefficients(float(d["beta"]), 2)
    A = {t: fixture_csr(d, t) for t in ("train", "full")}
    assert (A["train"] != A["full"]).nnz > 0 and not np.all(A["train"].data == 1.0)     # weighted, full != train
    for name in LISTS:
        pred = d[f"{name}_pred"]
        assert pred.dtype == np.float32
        truth = truncated_truth(A[GRAPH_OF[name]], d[f"{name}_edge"], coeffs).astype(np.float32)
        den = np.maximum(np.abs(truth), 1e-30)
        assert float((np.abs(pred.astype(np.float64) - truth) / den).max()) <= 1e-5, name
    # the textbook series (beta^2) is NOT what the reference computes
    textbook = truncated_truth(A["full"], d["pos_test_edge"], (0.05, 0.0025, 0.000125))
    assert not np.allclose(textbook, d["pos_test_pred"], rtol=1e-3)


def test_ddi_fixture_is_the_inverse(eps):
    d = load_fixture("katz_ddi_like.npz")
    assert str(d["dataset"]) == "ddi"
    cond = float(d["cond"])
    assert cond <= 1e6
    H = exact_truth(fixture_csr(d, "train"), float(d["beta"]))
    tol = exact_tolerance(cond, H)
    for name in LISTS:
        pred = d[f"{name}_pred"]
        assert pred.dtype == np.float64
        e = d[f"{name}_edge"]
        assert float(np.abs(pred - H[e[:, 0], e[:, 1]]).max()) <= tol, name


def test_katz_exports_refuse_bad_arguments_before_any_launch(eps):
    """EINVAL comes back (rc -1, with a message) before any HIP call: checkable without a GPU."""
    import ctypes
    lib = eps.load()
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: every call below must stop at its argument checks
    args = [fake] * 8
    # null pointers
    rc = lib.eps_katz_pair_scores(None, None, None, None, None, None, None, None, 10, None, None, 5, 0.05, 0.005, 0.000125,
                                  None, None, None)
    assert rc == -1 and b"null" in lib.eps_last_error()
    rc = lib.eps_katz_pair_scores(*args, 10, fake, fake, 5, 0.05, 0.005, 0.000125, None, fake, None)
    assert rc == -1 and b"null" in lib.eps_last_error()
    # negative sizes
    rc = lib.eps_katz_pair_scores(*args, -1, fake, fake, 5, 0.05, 0.005, 0.000125, fake, fake, None)
    assert rc == -1 and b"negative" in lib.eps_last_error()
    rc = lib.eps_katz_pair_scores(*args, 10, fake, fake, -5, 0.05, 0.005, 0.000125, fake, fake, None)
    assert rc == -1 and b"negative" in lib.eps_last_error()
    # non-finite coefficients
    for bad in (float("nan"), float("inf"), float("-inf")):
        rc = lib.eps_katz_pair_scores(*args, 10, fake, fake, 5, 0.05, bad, 0.000125, fake, fake, None)
        assert rc == -1 and b"non-finite" in lib.eps_last_error()
    # the two-path counts
    rc = lib.eps_two_path_counts(None, None, 10, None, None)
    assert rc == -1 and b"null" in lib.eps_last_error()
    rc = lib.eps_two_path_counts(fake, fake, -1, fake, None)
    assert rc == -1 and b"negative" in lib.eps_last_error()
    # an empty request is a no-op (rc 0), also without pointers
    assert lib.eps_katz_pair_scores(None, None, None, None, None, None, None, None, 0, None, None, 0, 0.0, 0.0, 0.0,
                                    None, None, None) == 0
    assert lib.eps_katz_workspace_bytes(0) == 0 and lib.eps_katz_workspace_bytes(1000) >= 1000 * 4


def test_exact_katz_refuses_large_graphs_before_touching_the_device(eps, monkeypatch):
    from eps_amd import heuristics
    n = heuristics.EXACT_KATZ_MAX_NODES + 1

    def no_device(*a, **k):
        raise AssertionError("exact_katz reached the device path above the cap")

    monkeypatch.setattr(heuristics, "_as_graph", no_device)
    monkeypatch.setattr(heuristics, "_default_device", no_device)
    A = ssp.identity(n, dtype=np.float32, format="csr")
    with pytest.raises(eps.EpsError, match=r"EXACT_KATZ_MAX_NODES.*GiB"):
        heuristics.exact_katz(A, np.zeros((2, 1), dtype=np.int64))
    g = eps.CSRGraph.from_scipy(ssp.identity(576_289, dtype=np.float32, format="csr"))      # the ppa stand-in's size
    with pytest.raises(eps.EpsError, match=r"4948\.\d GiB"):
        heuristics.exact_katz(g, np.zeros((2, 1), dtype=np.int64))
