"""CPU: the bf16 screening decode without a GPU -- the float64 emulation of eps_mlp_decode_bf16's rounding points (shared with
tests/test_gpu_decode_bf16.py), the filter stage's argument checks, the size of the screening pass, and the signature table."""
import argparse
import math

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------- the emulation
def rne_bf16_bits(x):
    """float32 array -> uint16 bfloat16 bit patterns, round to nearest, ties to even; every NaN -> 0x7FC0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(x)] = 0x7FC0
    return out


def bf16_to_f64(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def rne_bf16(x):
    """A float array rounded to bfloat16 (through float32), as float64 values."""
    with np.errstate(over="ignore"):
        return bf16_to_f64(rne_bf16_bits(np.asarray(x, dtype=np.float64).astype(np.float32)))


def emulate_decode_bf16(h_bits, u, v, ws, bs, acc=np.float64):
    """The logits of eps_mlp_decode_bf16 by its rounding points.  ``h_bits``: uint16 [N, H]; ``ws``: hidden layers as uint16 bf16
    bits [H, H], the last as float32 [1, H]; ``bs`` float32.  ``acc``: the accumulation type (float64: the reference; float32:
    what a kernel can do).  -> (logits float64 [E], sum of |terms| of the final dot + |bias| [E])."""
    h = bf16_to_f64(h_bits)
    x = rne_bf16(h[u] * h[v])                                  # exact product, one rounding
    L = len(ws)
    for l in range(L - 1):
        W = bf16_to_f64(ws[l])
        a = (x.astype(acc) @ W.T.astype(acc)).astype(acc) + np.asarray(bs[l]).astype(acc)
        a = np.maximum(a, 0).astype(np.float64)
        x = rne_bf16(a) if l < L - 2 else (a if acc is np.float64 else a.astype(np.float32).astype(np.float64))
    wl = np.asarray(ws[-1], dtype=np.float64).reshape(-1)
    terms = x * wl
    b_last = float(np.asarray(bs[-1]).reshape(-1)[0])
    if acc is np.float64:
        logit = terms.sum(1) + b_last
    else:
        logit = ((x.astype(np.float32) * wl.astype(np.float32)).sum(1, dtype=np.float32) + np.float32(b_last)).astype(np.float64)
    return logit, np.abs(terms).sum(1) + abs(b_last)


def special_vector():
    """Ties, +-0, subnormals, +-inf, NaNs, the largest finite float and 10^4 random floats (all exponents)."""
    rng = np.random.default_rng(7)
    ties = np.array([0x3F808000, 0x3F818000, 0x3F828000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x00008000, 0x00018000,
                     0x7F7F8000, 0x7F7F7FFF], dtype=np.uint32)                   # (0x7F7F8000: a tie that rounds to +inf)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00010000, 0x7F800000,
                        0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FBFFFFF, 0x7F7FFFFF, 0xFF7FFFFF],
                       dtype=np.uint32)
    rand = rng.integers(0, 1 << 32, 10_000, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([ties, special, rand]).view(np.float32)


def same_bf16_bits(got, want, x):
    """Bit for bit wherever ``x`` is a number; NaN for NaN elsewhere (see test_rne_helper_matches_torch_bit_for_bit)."""
    got, want = np.asarray(got).view(np.uint16).ravel(), np.asarray(want).view(np.uint16).ravel()
    nan = np.isnan(np.asarray(x, dtype=np.float32).ravel())
    return (np.array_equal(got[~nan], want[~nan]) and bool(np.isnan(bf16_to_f64(got[nan])).all())
            and bool(np.isnan(bf16_to_f64(want[nan])).all()))


def test_rne_helper_matches_torch_bit_for_bit():
    x = special_vector()
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = rne_bf16_bits(x)
    nan = np.isnan(x)
    assert nan.sum() >= 5 and np.array_equal(got[~nan], want[~nan])
    # a NaN stays a NaN.  Its bits are not compared: torch has no single answer (c10's scalar rounding gives 0x7FC0, the
    # vectorised CPU conversion 0xFFFF); the library and this helper give 0x7FC0
    assert bool(np.isnan(bf16_to_f64(got[nan])).all()) and bool(np.isnan(bf16_to_f64(want[nan])).all())
    assert bool((got[nan] == 0x7FC0).all())
    assert got[0] == 0x3F80 and got[1] == 0x3F82 and got[2] == 0x3F82           # ties go to the even neighbour


def test_emulation_rounds_where_the_kernel_rounds():
    """Two nodes, H = 16, L = 3, values chosen so that each rounding point changes the result."""
    H = 16
    h = np.zeros((2, H), np.float32)
    h[0, 0], h[1, 0] = 1.0078125, 1.0078125          # (1 + 2^-7)^2 = 1 + 2^-6 + 2^-14 -> bf16 1.015625
    hb = rne_bf16_bits(h)
    w1 = np.zeros((H, H), np.float32); w1[0, 0] = 1.0
    w2 = np.zeros((H, H), np.float32); w2[0, 0] = 1.0
    wl = np.zeros((1, H), np.float32); wl[0, 0] = 1.0
    b1 = np.zeros(H, np.float32); b1[0] = 2.0 ** -9  # a quarter of a bf16 step at 1.0: rounded away after the first hidden layer
    b2 = np.zeros(H, np.float32); b2[0] = 2.0 ** -12
    bl = np.zeros(1, np.float32)
    logit, tsum = emulate_decode_bf16(hb, np.array([0]), np.array([1]), [rne_bf16_bits(w1), rne_bf16_bits(w2), wl], [b1, b2, bl])
    x0 = 1.015625
    a1 = float(rne_bf16(np.array([x0 + 2.0 ** -9]))[0])          # first hidden layer: rounded to bf16
    assert a1 == 1.015625
    assert logit[0] == a1 + 2.0 ** -12                           # last hidden layer: NOT rounded
    assert tsum[0] == abs(logit[0])


# ---------------------------------------------------------------------------------------------- the filter stage's checks
def _args(**kw):
    from eps_amd import filter_stage, models
    base = ["--dataset", "ddi", "--model", "gcn", "--checkpoint", "ddi_gcn||0|0.pt", "--synthetic"]
    a = filter_stage.make_parser().parse_args(base)
    for k, v in kw.items():
        setattr(a, k, v)
    return models.default_model_configs(a)


def test_default_command_line_is_fp32():
    from eps_amd import filter_stage
    a = _args()
    assert a.decode_precision == "fp32" and a.decode_guard is None
    filter_stage.check_decode_args(a)                          # the bare command: nothing to refuse
    filter_stage.check_decode_args(_args(model="adamic_ogb", keep_top=100))
    ok = _args(keep_top=1000, decode_precision="bf16")
    filter_stage.check_decode_args(ok)
    filter_stage.check_decode_args(_args(keep_top=1000, decode_precision="bf16", decode_guard=1.0, model="dea"))


@pytest.mark.parametrize("kw,word", [
    (dict(model="adamic_ogb", keep_top=1000, decode_precision="bf16"), "adamic_ogb"),
    (dict(decode_precision="bf16"), "--keep_top"),
    (dict(keep_top=1000, decode_precision="bf16", decode_guard=0.5), "G >= 1"),
    (dict(keep_top=1000, decode_precision="bf16", decode_guard=float("nan")), "G >= 1"),
    (dict(model="dea_512", keep_top=1000, decode_precision="bf16"), "512"),
    (dict(keep_top=1000, decode_precision="bf16", hidden_channels=300), "300"),
    (dict(keep_top=1000, decode_precision="bf16", num_layers=1), "one-layer"),
    (dict(keep_top=1000, decode_guard=2.0), "--decode_guard"),
])
def test_unserved_combinations_are_refused_with_a_message(kw, word):
    from eps_amd import filter_stage
    with pytest.raises(ValueError, match=word.replace("(", r"\(")):
        filter_stage.check_decode_args(_args(**kw))


def test_refusal_comes_before_the_dataset_is_read(monkeypatch):
    """run() checks the flags right after the model defaults are filled in: get_data is never reached."""
    from eps_amd import filter_stage

    def boom(*a, **k):
        raise AssertionError("the dataset was read")
    monkeypatch.setattr(filter_stage, "get_data", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    with pytest.raises(ValueError, match="adamic_ogb"):
        filter_stage.main(["--dataset", "ddi", "--model", "adamic_ogb", "--checkpoint", "x||0|0.pt", "--synthetic",
                           "--keep_top", "10", "--decode_precision", "bf16"])


def test_sharded_runs_are_refused(monkeypatch):
    from eps_amd import filter_stage
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process"):
        filter_stage.check_decode_args(_args(keep_top=1000, decode_precision="bf16"))


@pytest.mark.parametrize("K,G,M", [(1000, 1.0, 500), (1001, 1.0, 501), (1000, 1.25, 625), (7, 1.5, 6), (50, 4.0, 100),
                                   (1, 1.0, 1), (3, 1.1, 3), (200, 1e9, 100 * 10 ** 9)])
def test_screen_size(K, G, M):
    from eps_amd import filter_stage
    assert filter_stage.screen_size(K, G) == M == math.ceil(G * math.ceil(K / 2))


def test_default_guard_is_a_guard():
    from eps_amd import filter_stage
    assert filter_stage.DECODE_GUARD_DEFAULT >= 1.0
    assert f"{filter_stage.DECODE_GUARD_DEFAULT:g}" in filter_stage.make_parser().format_help()


# ---------------------------------------------------------------------------------------------- bindings
def test_signatures_hold_both_exports_and_agree_with_the_header(eps):
    import test_abi
    from eps_amd import ops
    assert ops.SIGNATURES is eps._lib.SIGNATURES
    for name in ("eps_mlp_decode_bf16", "eps_f32_to_bf16"):
        assert name in ops.SIGNATURES and name in test_abi.declared_symbols()
    protos = test_abi.declared_prototypes()
    for name in ("eps_mlp_decode_bf16", "eps_f32_to_bf16"):
        ret, kinds = protos[name]
        res, args = ops.SIGNATURES[name]
        assert test_abi._ctypes_kind(res) == ret and [test_abi._ctypes_kind(a) for a in args] == kinds
    test_abi.test_python_signatures_cover_header(eps)          # the whole table, by the existing checker
    assert callable(ops.to_bf16) and callable(ops.mlp_decode_bf16)


def test_argument_validation_without_gpu(eps):
    """The shape checks return before any HIP call."""
    lib = eps.load()
    for hd, L, word in [(20, 2, b"hdim"), (272, 2, b"hdim"), (512, 2, b"hdim"), (300, 3, b"hdim"), (256, 1, b"n_layers"), (256, 9, b"n_layers")]:
        rc = lib.eps_mlp_decode_bf16(None, 0, hd, None, None, 0, None, None, L, 0, None, None)
        assert rc == -1 and word in lib.eps_last_error(), (hd, L)
    assert lib.eps_f32_to_bf16(None, -1, None, None) == -1
    assert lib.eps_f32_to_bf16(None, 0, None, None) == 0


def test_ops_refuse_cpu_and_wrong_dtypes(eps):
    from eps_amd import ops
    with pytest.raises(eps.EpsError):
        ops.to_bf16(torch.zeros(4))
    with pytest.raises(eps.EpsError):
        ops.mlp_decode_bf16(torch.zeros(4, 16, dtype=torch.int16), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                            [torch.zeros(16, 16, dtype=torch.int16), torch.zeros(1, 16)], [torch.zeros(16), torch.zeros(1)])


def test_decode_precision_argument_is_checked():
    from eps_amd import models
    lp = models.LinkPredictor(16, 16, 1, 2, 0.0)
    with pytest.raises(ValueError, match="fp16"):
        lp.decode(torch.zeros(4, 16), torch.zeros(2, 1, dtype=torch.int64), precision="fp16")
