"""What tests/test_decode_bn_host.py (CPU) and tests/test_gpu_decode_bn.py (GPU) share: the small cases of DEA_GNN_JK's
two-layer decoder (decode_train_cases.make_case plus a BatchNorm weight in 0.5 .. 1.5 and a bias), the restatement of its training
forward WITH a dropout mask in the dtype of its inputs (float64 = the truth, float32 = the plain dense torch formulation; the
BatchNorm written out: batch mean, biased variance, eps inside the root), and the gradients of training_truth.bce_logits_loss
through it.  The gradient protocol is decode_train_cases.check_grads.  A plain helper module, no fixtures."""
import torch

import decode_train_cases as dc
import training_truth as tt

HS = (32, 36, 64, 256)          # the minimum, pad columns, a whole tile row of waves idle, the full tile
BS = (2, 63, 64, 65, 200)       # the smallest legal batch and the 64-edge tile boundary
SHAPES = [(H, B) for H in HS for B in BS]


def seed_of(H, B):
    return 1000 * H + 10 * B + 7


def make_case(H, B, seed, p_drop=0.5, h_shift=0.0, h_scale=1.0, zero_row=None):
    """CPU float32 case -> (h, edges, ws, bs, gamma, beta, keep): dc.make_case(H, 2, B, seed) with keep [B, H], gamma uniform in
    0.5 .. 1.5, beta normal * 0.1.  ``h_shift`` / ``h_scale``: h <- h * h_scale + h_shift (a batch whose pre-activations sit far
    from 0 in units of their spread).  ``zero_row``: that row of W0 is zeroed (a channel of variance 0)."""
    h, edges, ws, bs, keep = dc.make_case(H, 2, B, seed, p_drop)
    g = torch.Generator().manual_seed(seed + 1)
    gamma = torch.rand(H, generator=g) + 0.5
    beta = torch.randn(H, generator=g) * 0.1
    h = h * h_scale + h_shift
    if zero_row is not None:
        ws[0][zero_row] = 0.0
    return h, edges, ws, bs, gamma, beta, keep[0]


def statistics(h, edges, ws, bs):
    """(mean, biased variance) [H] of z = (h[u] * h[v]) W0^T + b0 over the batch, in the inputs' dtype."""
    z = (h[edges[0]] * h[edges[1]]) @ ws[0].t() + bs[0]
    return z.mean(0), z.var(0, unbiased=False)


def bn_forward(h, edges, ws, bs, gamma, beta, keep=None, scale=1.0, branch=None, pre=None, eps=tt.BN_EPS):
    """Hadamard -> Linear -> BatchNorm on batch statistics -> ReLU -> keep * scale -> Linear -> logits [B].  ``branch`` (one
    boolean [B, H] mask) / ``pre`` (a list that collects the ReLU's input): as in training_truth._relu."""
    z = (h[edges[0]] * h[edges[1]]) @ ws[0].t() + bs[0]
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    y = gamma * (z - mu) / torch.sqrt(var + eps) + beta
    a = tt._relu(y, None if branch is None else iter([branch]), pre)
    if keep is not None:
        a = a * (keep.to(a.dtype) * scale)
    return (a @ ws[1].t() + bs[1]).squeeze(1)


def labels(B):
    """The first half of the batch are positives."""
    return torch.cat([torch.ones(B // 2), torch.zeros(B - B // 2)])


def reference_grads(h, edges, ws, bs, gamma, beta, keep, scale, branch, dtype):
    """{name: grad} of bce_logits_loss(bn_forward(...), labels) in ``dtype`` on the given ReLU branch: 'h', 'w0', 'w1', 'b0',
    'b1', 'gamma', 'beta'."""
    leaf = lambda x: x.detach().to(dtype).clone().requires_grad_(True)   # noqa: E731
    hh, w, b, ga, be = leaf(h), [leaf(x) for x in ws], [leaf(x) for x in bs], leaf(gamma), leaf(beta)
    out = bn_forward(hh, edges, w, b, ga, be, keep, scale, branch=branch)
    tt.bce_logits_loss(out, labels(out.numel())).backward()
    return {"h": hh.grad, "w0": w[0].grad, "w1": w[1].grad, "b0": b[0].grad, "b1": b[1].grad, "gamma": ga.grad, "beta": be.grad}


def own_branch(h, edges, ws, bs, gamma, beta, keep, scale):
    """The ReLU branch float64 itself takes."""
    pre = []
    d = torch.float64
    with torch.no_grad():
        bn_forward(h.to(d), edges, [w.to(d) for w in ws], [b.to(d) for b in bs], gamma.to(d), beta.to(d), keep, scale, pre=pre)
    return pre[0] > 0
