"""CPU: the float64 truth of the GNN training path (tests/training_truth.py) is itself checked here -- its forwards against the
oracle's dense formulas, its closed-form SpMM backward against torch autograd, and the reason models._SpMM needs a symmetric
adjacency (the shortcut A dY is far from A^T dY on an asymmetric one) -- next to properties of training.negative_sampling."""
import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import training_truth as tt


def small_graph(n=40, m=160, seed=0, symmetric=True, loops=True):
    """Weighted graph (integer weights summed over duplicate edges), stored self loops on some nodes, node n-1 isolated."""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n - 1, m), rng.integers(0, n - 1, m)
    w = rng.integers(1, 5, m).astype(np.float64)
    if not loops:
        keep = r != c
        r, c, w = r[keep], c[keep], w[keep]
    A = ssp.coo_matrix((w, (r, c)), shape=(n, n)).tocsr()
    if symmetric:
        A = (A + A.T).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    assert A[n - 1].nnz == 0 and A[:, n - 1].nnz == 0
    return A


def test_forward_agrees_with_the_oracle(oracle):
    A = small_graph()
    n = A.shape[0]
    Ad = A.toarray()
    assert (Ad == Ad.T).all() and Ad.diagonal().max() > 1 and (Ad.diagonal() == 0).any()   # stored loops (values != 1), not on every node
    rng = np.random.default_rng(1)
    dims = [7, 6, 6, 5]
    x = rng.standard_normal((n, dims[0]))
    At = torch.from_numpy(Ad)
    # GCN: [in, out] weights
    ws = [rng.standard_normal((dims[i], dims[i + 1])) for i in range(3)]
    bs = [rng.standard_normal(dims[i + 1]) for i in range(3)]
    got = tt.gcn_stack(tt.gcn_matrix(At), torch.from_numpy(x), [torch.from_numpy(w) for w in ws], [torch.from_numpy(b) for b in bs])
    ref = oracle.gcn_dense_forward(Ad, x, ws, bs)
    assert got.dtype == torch.float64
    assert float(np.abs(got.numpy() - ref).max()) <= 1e-13 * float(np.abs(ref).max())
    # SAGE: Linear layout [out, in]; the mean runs over the pattern and ignores the values
    wl = [rng.standard_normal((dims[i + 1], dims[i])) for i in range(3)]
    bl = [rng.standard_normal(dims[i + 1]) for i in range(3)]
    wr = [rng.standard_normal((dims[i + 1], dims[i])) for i in range(3)]
    P = (At != 0).double()
    t = lambda xs: [torch.from_numpy(a) for a in xs]
    got = tt.sage_stack(tt.mean_matrix(P), torch.from_numpy(x), t(wl), t(bl), t(wr))
    ref = oracle.sage_dense_forward(Ad, x, wl, bl, wr)
    assert float(np.abs(got.numpy() - ref).max()) <= 1e-13 * float(np.abs(ref).max())
    # the isolated node's mean is 0 (degree clamped to 1): layer 1 there is lin_r(x) + b alone
    one = tt.sage_stack(tt.mean_matrix(P), torch.from_numpy(x), t(wl[:1]), t(bl[:1]), t(wr[:1])).numpy()
    assert np.allclose(one[n - 1], x[n - 1] @ wr[0].T + bl[0], rtol=0, atol=1e-13)


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("symmetric", [True, False])
def test_closed_form_backward_agrees_with_autograd(mean, symmetric):
    A = small_graph(seed=2, symmetric=symmetric)
    n = A.shape[0]
    rng = np.random.default_rng(3)
    X = torch.from_numpy(rng.standard_normal((n, 9))).requires_grad_(True)
    G = rng.standard_normal((n, 9))
    Ad = torch.from_numpy(A.toarray())
    M = tt.mean_matrix((Ad != 0).double()) if mean else Ad
    Y = M @ X
    assert float(np.abs(Y.detach().numpy() - tt.spmm_forward(A, X.detach().numpy(), mean)).max()) <= 1e-13 * float(Y.detach().abs().max())
    (Y * torch.from_numpy(G)).sum().backward()
    closed = tt.spmm_backward(A, G, mean)
    scale = float(X.grad.abs().max())
    assert float(np.abs(closed - X.grad.numpy()).max()) <= 1e-13 * scale
    short = tt.spmm_backward_shortcut(A, G, mean)
    if symmetric:                                   # ... and then the product with A itself IS the gradient
        assert float(np.abs(short - closed).max()) <= 1e-13 * scale


@pytest.mark.parametrize("mean", [False, True])
def test_shortcut_is_wrong_on_an_asymmetric_matrix(mean):
    """models._SpMM.backward computes A dY.  On a directed graph that is a different vector from the gradient A^T dY: not a
    rounding difference but one of the size of the gradient itself -- which is why the convs refuse such a graph in training."""
    A = small_graph(n=60, m=300, seed=4, symmetric=False)
    assert (A != A.T).nnz > 100
    G = np.random.default_rng(5).standard_normal((60, 16))
    true, short = tt.spmm_backward(A, G, mean), tt.spmm_backward_shortcut(A, G, mean)
    assert float(np.abs(short - true).max()) >= 0.5 * float(np.abs(true).max())
    assert float(np.linalg.norm(short - true)) >= 0.5 * float(np.linalg.norm(true))


def test_shortcut_is_wrong_on_asymmetric_values_for_sum_only():
    """A symmetric pattern with asymmetric values: the sum's shortcut is wrong, the mean's (which never reads the values) is
    exact -- GCNConv / TAGConv must refuse this graph in training, SAGEConv must take it."""
    A = small_graph(seed=6, loops=False)
    A = A.tocsr().astype(np.float64)
    U = ssp.triu(A, 1).tocsr()
    B = (A + 3.0 * U).tocsr()                       # upper triangle x4, lower untouched: same pattern
    B.sort_indices()
    assert (tt.pattern_of(B) != tt.pattern_of(B).T).nnz == 0 and (B != B.T).nnz > 50
    G = np.random.default_rng(7).standard_normal((B.shape[0], 8))
    true, short = tt.spmm_backward(B, G, False), tt.spmm_backward_shortcut(B, G, False)
    assert float(np.abs(short - true).max()) >= 0.5 * float(np.abs(true).max())
    assert float(np.abs(tt.spmm_backward_shortcut(B, G, True) - tt.spmm_backward(B, G, True)).max()) <= 1e-13 * float(np.abs(G).max())


def test_losses_match_the_training_loop():
    g = torch.Generator().manual_seed(8)
    out = torch.rand(40, generator=g, dtype=torch.float64)
    ref = -torch.log(out[:25] + 1e-8).mean() - torch.log(1 - out[25:] + 1e-8).mean()       # training.train, gcn / sage
    assert float(tt.log_loss(out, 25) - ref) == 0.0
    logits = torch.randn(40, generator=g, dtype=torch.float64)
    label = torch.cat([torch.ones(25), torch.zeros(15)])
    ref = torch.nn.BCEWithLogitsLoss()(logits, label.double())                               # DEA_GNN_JK.loss
    assert abs(float(tt.bce_logits_loss(logits, label) - ref)) <= 1e-15


# ---------------------------------------------------------------------------------------------------------- negative_sampling
def _check_negatives(neg, ei, n, count):
    assert neg.shape == (2, count) and neg.dtype == torch.int64                 # the count is exact
    if count:
        assert int(neg.min()) >= 0 and int(neg.max()) < n                       # ids in range
    edge_keys = set((ei[0] * n + ei[1]).tolist())
    assert not (set((neg[0] * n + neg[1]).tolist()) & edge_keys)                # no output is an edge


@pytest.mark.parametrize("count", [0, 1, 17, 1000, 5000])
def test_negative_sampling_on_a_dense_graph(eps, count):
    """Well over half of all pairs are edges: most draws are rejected, the loop still returns exactly ``count`` non-edges."""
    from eps_amd import training
    n = 40
    g = torch.Generator().manual_seed(9)
    keep = torch.rand(n * n, generator=g) < 0.85
    keys = torch.arange(n * n)[keep]
    ei = torch.stack([keys // n, keys % n])
    assert ei.shape[1] > 0.8 * n * n
    torch.manual_seed(10)
    _check_negatives(training.negative_sampling(ei, n, count), ei, n, count)


@pytest.mark.parametrize("n", [1, 2, 50])
def test_negative_sampling_without_edges(eps, n):
    from eps_amd import training
    ei = torch.zeros((2, 0), dtype=torch.int64)
    torch.manual_seed(11)
    neg = training.negative_sampling(ei, n, 300)
    _check_negatives(neg, ei, n, 300)
    if n == 1:
        assert int(neg.abs().max()) == 0                                         # the only pair there is
