"""GPU: the bf16 BasicBlock conv pair (po2q_qconv2d_pair_bf16, conv_b16_pair<C, GW>) through the C ABI, y between
sentinel bands.

Contract (include/po2q.h): mid = bf16(act1((acc1 + b1) s1 + t1)), y = bf16(act2((acc2 + b2) s2 + t2 + x)), i.e. two
po2q_qconv2d_fused_bf16 calls with residual = x up to the accumulation order; conv 2 pads with zeros.

Exact operands: x integers in [-2, 2]; mode none weights integers / 8 in [-1, 1], po2 / po2+ at bits = 3 with one
weight 1.0, so Q(w) is one of 1/8, 1/4, 1/2, 1 (asserted); biases integers / 8.  Conv-1 sums are multiples of 1/8
below 2^10, conv-2 sums multiples of 1/64 below 576 * 288 < 2^18: exact in fp32 in any order, so the kernel has
to give the bits of the fp64 chain with mid rounded to bf16, and those of the two fused calls.

Random operands: the bar chains tests/test_gpu_bf16_fused.py's fused_ref_bar over both layers.  With u = 2^-8,
k = 9 C: (ref1, tol1) = fused_ref_bar(c1, mag1, k, s1, t1, None, act1); c2 = conv(ref1, Q2) + b2,
D = conv(tol1, |Q2|), mag2 = conv(|ref1| + tol1, |Q2|) + |b2|; (ref2, tol2) = fused_ref_bar(c2, mag2, k, s2, t2,
x if add_x, act2); bound = tol2 + (1 + u) lip |s2| D.  D carries mid's rounding (about 2^-8 of the magnitude); a
misplaced tap is of the order of the magnitude itself."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from po2_quantization_amd import _lib
from po2_quantization_amd.models import quantized_conv as qc
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.models.resnet import BasicBlock
from po2_quantization_amd.utils.quantizers import NATIVE_MODES, quantizer_dict
from tests import test_gpu_bf16_conv_paths as paths
from tests import test_gpu_bf16_fused as fz
from tests._bf16_cases import BF, random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, 0x5a5a
# (N, C, H, W): both C; W = 2, 18 (ragged group, idle waves), 34 (GW 1, three groups), 70 (GW 2 ragged), 130 (GW 4),
# Wmax; H = 1, 2, 3 (every mid row at or next to the image edge); H = 5, 9 at RB = 4 (several bands, a one-row last
# band, band-edge mid rows inside the image); N = 3
TABLE = [(2, 16, 1, 2), (3, 16, 2, 18), (2, 32, 3, 34), (2, 32, 5, 70), (2, 16, 9, 70), (1, 16, 9, 130), (1, 16, 9, 256),
         (1, 32, 3, 128), (3, 32, 9, 18), (1, 16, 5, 34), (2, 32, 1, 2), (1, 32, 2, 128)]
TABLE_P = pytest.mark.parametrize("shape", TABLE, ids=lambda s: "x".join(map(str, s)))


def dev(*ts):
    return tuple(t.to(DEV) if t is not None else None for t in ts)


def bits_of(t):
    return t.contiguous().view(torch.int16)


def s13(shape):
    return (shape[0], shape[1], shape[2], shape[3], shape[1], 3, 3, 1, 1, 1, 1, 1, 1)


def run_pair(x, w1, w2, shape, mode, bits, b1=None, b2=None, s1=None, t1=None, act1=0, s2=None, t2=None, add_x=0, act2=0,
             y_shift=0, ws_cut=0):
    """po2q_qconv2d_pair_bf16 on device tensors as they are; y starts y_shift elements past an 8-byte aligned address
    inside a guard buffer.  Returns (status, y on the CPU or None) after checking both guard bands; a refused call
    has to leave y untouched as well."""
    L = _lib.load()
    n = x.numel()
    mode_id = fz.MODE_ID[mode]
    need = L.po2q_qconv2d_pair_bf16_workspace_bytes(*shape, bits, 1, mode_id)
    assert need > 0, L.po2q_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    buf = torch.full((GUARD + 4 + n + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    y = buf[GUARD + y_shift:GUARD + y_shift + n]
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    st = L.po2q_qconv2d_pair_bf16(x.data_ptr(), w1.data_ptr(), w2.data_ptr(), y.data_ptr(), *shape, bits, 1, mode_id,
                                  p(b1), p(b2), p(s1), p(t1), act1, p(s2), p(t2), add_x, act2, ws.data_ptr(),
                                  need - ws_cut, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = buf.cpu()
    body = out[GUARD + y_shift:GUARD + y_shift + n]
    assert bool((out[:GUARD + y_shift] == SENTINEL).all()) and bool((out[GUARD + y_shift + n:] == SENTINEL).all()), "guard band written"
    if st != 0:
        assert bool((body == SENTINEL).all()), "a refused call wrote y"
        return st, None
    return st, body.view(BF).view(shape)


def two_calls(x, w1, w2, shape, mode, bits, b1, b2, s1, t1, act1, s2, t2, add_x, act2):
    """The two po2q_qconv2d_fused_bf16 calls the pair replaces (residual = x)."""
    L = _lib.load()
    g = s13(shape) + (1,)
    need = L.po2q_qconv2d_bf16_workspace_bytes(*g, bits, 1, fz.MODE_ID[mode])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    mid, y = torch.empty_like(x), torch.empty_like(x)
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for src, w, b, s, t, res, act, dst in ((x, w1, b1, s1, t1, None, act1, mid), (mid, w2, b2, s2, t2, x if add_x else None, act2, y)):
        st = L.po2q_qconv2d_fused_bf16(src.data_ptr(), w.data_ptr(), p(b), dst.data_ptr(), *g, bits, 1, fz.MODE_ID[mode], p(s),
                                       p(t), p(res), act, ws.data_ptr(), need, stream)
        assert st == 0, L.po2q_last_error()
    torch.cuda.synchronize()
    return y.cpu()


def exact_operands(shape, mode, bias, seed):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, shape, generator=g).to(BF)
    ws = []
    for _ in range(2):
        if mode == "none":
            w = (torch.randint(-8, 9, (C, C, 3, 3), generator=g).float() / 8).to(BF)
        else:
            w = (torch.rand(C, C, 3, 3, generator=g) * 2 - 1).to(BF)
            w.view(-1)[0] = 1.0
            assert set(_lib.restated_quantize(w, 3, mode).float().abs().unique().tolist()) <= {0.125, 0.25, 0.5, 1.0}
        ws.append(w)
    bs = [(torch.randint(-8, 9, (C,), generator=g).float() / 8).to(BF) if bias else None for _ in range(2)]
    return x, ws[0], ws[1], bs[0], bs[1]


def chain64(x, q1, q2, b1, b2, act1, act2, add_x):
    """The fp64 chain with mid rounded to bf16 (no affine)."""
    d = lambda t: t.double() if t is not None else None  # noqa: E731
    mid = fz.act64(F.conv2d(x.double(), q1.double(), d(b1), 1, 1), act1).to(BF)
    return fz.act64(F.conv2d(mid.double(), q2.double(), d(b2), 1, 1) + (x.double() if add_x else 0.0), act2)


def pair_bound(x, q1, q2, b1, b2, s1, t1, act1, s2, t2, add_x, act2):
    """(ref2, bound) of the module docstring: fused_ref_bar chained over both layers."""
    k = 9 * x.shape[1]
    d = lambda t: t.double() if t is not None else None  # noqa: E731
    c1, mag1 = fz.reference(x, q1, b1, 1, 1, 1, 1)
    ref1, tol1 = fz.fused_ref_bar(c1, mag1, k, s1, t1, None, act1)
    q2a = q2.double().abs()
    c2 = F.conv2d(ref1, q2.double(), d(b2), 1, 1)
    D = F.conv2d(tol1, q2a, None, 1, 1)
    mag2 = F.conv2d(ref1.abs() + tol1, q2a, d(b2).abs() if b2 is not None else None, 1, 1)
    ref2, tol2 = fz.fused_ref_bar(c2, mag2, k, s2, t2, x if add_x else None, act2)
    s2a = s2.double().abs().view(1, -1, 1, 1) if s2 is not None else 1.0
    return ref2, tol2 + (1 + 2.0 ** -8) * (1.1 if act2 == "silu" else 1.0) * s2a * D


@pytest.mark.parametrize("bias,act2,add_x", [(True, "relu", 1), (False, "none", 0), (True, "none", 1)], ids=["b-relu-x", "plain", "b-none-x"])
@pytest.mark.parametrize("mode", ["po2", "po2+", "none"])
@TABLE_P
def test_bit_exact_with_the_fp64_chain_and_the_two_fused_calls(shape, mode, bias, act2, add_x):
    x, w1, w2, b1, b2 = exact_operands(shape, mode, bias, 61)
    q1, q2 = (w if mode == "none" else _lib.restated_quantize(w, 3, mode) for w in (w1, w2))
    ref = chain64(x, q1, q2, b1, b2, "relu", act2, add_x).to(BF)
    args = dev(x, w1, w2) + (shape, mode, 3) + dev(b1, b2) + (None, None, 1, None, None, add_x, fz.ACT_ID[act2])
    st, y = run_pair(*args)
    assert st == 0, _lib.load().po2q_last_error()
    assert torch.equal(bits_of(y), bits_of(ref)), "%d of %d elements differ from the reference" % (int((y != ref).sum()), y.numel())
    two = two_calls(*args)
    assert torch.equal(bits_of(y), bits_of(two)), "%d elements differ from the two fused calls" % int((y != two).sum())


@pytest.mark.parametrize("mode,act1,act2", [("po2", "relu", "relu"), ("po2+", "relu6", "silu"), ("none", "silu", "relu6")])
@TABLE_P
def test_random_operands_error_bar(shape, mode, act1, act2):
    C = shape[1]
    x, w1, b1 = random_case(s13(shape), 1, 62, True)
    _, w2, b2 = random_case(s13(shape), 1, 63, True)
    g = torch.Generator().manual_seed(64)
    s1, t1, s2, t2 = (torch.randn(C, generator=g) for _ in range(4))
    q1, q2 = (w if mode == "none" else _lib.restated_quantize(w, 4, mode) for w in (w1, w2))
    ref, bound = pair_bound(x, q1, q2, b1, b2, s1, t1, act1, s2, t2, True, act2)
    args = dev(x, w1, w2) + (shape, mode, 4) + dev(b1, b2, s1, t1) + (fz.ACT_ID[act1],) + dev(s2, t2) + (1, fz.ACT_ID[act2])
    st, y = run_pair(*args)
    assert st == 0, _lib.load().po2q_last_error()
    err = (y.double() - ref).abs()
    two = two_calls(*args)
    print("%s %s worst err / bar = %.3f; %.4f of the elements differ from the two fused calls"
          % (shape, mode, (err / bound.clamp_min(1e-300)).max().item(), (y != two).float().mean().item()))
    assert bool(torch.isfinite(y.float()).all()) and bool((err <= bound).all())


@pytest.mark.parametrize("which", ["x", "y"])
@pytest.mark.parametrize("shape", [TABLE[4], TABLE[3]], ids=["16x70", "32x70"])
def test_two_byte_aligned_pointers(shape, which):
    x, w1, b1 = random_case(s13(shape), 1, 65, True)
    _, w2, b2 = random_case(s13(shape), 1, 66, True)
    x, w1, w2, b1, b2 = dev(x, w1, w2, b1, b2)
    _, want = run_pair(x, w1, w2, shape, "po2", 4, b1, b2, act1=1, add_x=1, act2=1)
    _, got = run_pair(paths.displaced(x) if which == "x" else x, w1, w2, shape, "po2", 4, b1, b2, act1=1, add_x=1, act2=1,
                      y_shift=1 if which == "y" else 0)
    assert torch.equal(bits_of(got), bits_of(want)), "%d elements differ" % int((got != want).sum())


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["pinf", "ninf", "nan"])
@pytest.mark.parametrize("where", ["corner", "band_edge", "group_edge"])
@pytest.mark.parametrize("shape", [TABLE[4], TABLE[8]], ids=["16x9x70", "32x9x18"])
def test_one_nonfinite_activation(shape, where, value):
    """RB = 4 at these shapes: rows 3 / 4 are a band edge.  The NaN / inf pattern is that of the fp64 chain (every
    Q(w) is nonzero); zero padding must add no NaN."""
    assert "RB=4 " in _lib.describe_pair_bf16(*shape)
    x, w1, b1 = random_case(s13(shape), 1, 67, True)
    _, w2, b2 = random_case(s13(shape), 1, 68, True)
    h, wc = {"corner": (0, 0), "band_edge": (3, 5), "group_edge": (5, 15)}[where]
    x = x.clone()
    x[shape[0] - 1, 5, h, wc] = value
    q1, q2 = _lib.restated_quantize(w1, 4, "po2"), _lib.restated_quantize(w2, 4, "po2")
    assert bool((q1 != 0).all()) and bool((q2 != 0).all())
    ref = chain64(x, q1, q2, b1, b2, "none", "relu", 1)
    st, y = run_pair(*dev(x, w1, w2), shape, "po2", 4, *dev(b1, b2), act1=0, add_x=1, act2=1)
    assert st == 0 and torch.equal(paths.kind(y), paths.kind(ref)), "NaN / inf pattern: %d elements differ" % int((paths.kind(y) != paths.kind(ref)).sum())
    assert not bool(torch.isfinite(ref).all()) and bool(torch.isfinite(ref).any())


def test_short_workspace_is_refused():
    shape = TABLE[1]
    x, w1, _ = dev(*random_case(s13(shape), 1, 69, False))
    st, y = run_pair(x, w1, w1, shape, "po2", 4, ws_cut=1)
    assert st == 3 and y is None and b"workspace" in _lib.load().po2q_last_error()  # PO2Q_ERR_WORKSPACE


def test_resnet20_forward_with_pairs(monkeypatch):
    """Every identity block of stages 1 and 2 takes the pair: its two convs leave the forward's batched-pack record.
    Per block (the pair's layer) the output meets pair_bound on the block's own input, the way
    tests/test_gpu_bf16_conv.py::test_model_layers bounds each conv; the logits difference is printed, not asserted
    (the layers' roundings compound)."""
    monkeypatch.setattr(qc, "BF16_FUSED_EPILOGUE", True)
    torch.manual_seed(19)
    model = get_model("resnet20", 10, quantizer_dict["po2"], 4, (32, 32)).eval().bfloat16().to(DEV)
    x = torch.randn(2, 3, 32, 32).to(BF).to(DEV)
    blocks = [m for m in model.modules() if isinstance(m, BasicBlock) and m.downsample is None and m.conv1.in_channels < 64]
    assert len(blocks) == 5
    with torch.no_grad():
        off = model(x)
        n_off = len(qc._RECORDS[model][qc._record_key(model, x)])
        monkeypatch.setattr(qc, "BF16_PAIRS", True)
        rec = []
        hooks = [b.register_forward_hook(lambda m, i, o: rec.append((m, i[0].cpu(), o.cpu()))) for b in blocks]
        on = [model(x), model(x)]
        for h in hooks:
            h.remove()
        n_on = len(qc._RECORDS[model][qc._record_key(model, x)])
    assert n_off - n_on == 2 * len(blocks) and torch.equal(bits_of(on[0]), bits_of(on[1]))
    print("max |logits(pairs) - logits(two calls)| = %.4g of max |logits| = %.4g"
          % ((on[0].float() - off.float()).abs().max().item(), off.float().abs().max().item()))
    assert bool(torch.isfinite(on[0].float()).all())
    for m, xi, yo in rec[:len(blocks)]:
        assert m._pair_bf16_ok(xi.to(DEV)) and _lib.describe_pair_bf16(*xi.shape).startswith("kind=bf16_pair ")
        mode = NATIVE_MODES[m.conv1.quantize_fn]
        q1, q2 = (_lib.restated_quantize(c.weight.detach().cpu(), c.bits, mode) for c in (m.conv1, m.conv2))
        (s1, t1), (s2, t2) = ((t.cpu() for t in qc.fold_bn_f32(bn)) for bn in (m.bn1, m.bn2))
        ref, bound = pair_bound(xi, q1, q2, None, None, s1, t1, "relu", s2, t2, True, "relu")
        assert bool(((yo.double() - ref).abs() <= bound).all()), tuple(xi.shape)
