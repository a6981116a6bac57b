"""GPU: the native bf16 conv forward (po2q_qconv2d_bf16) against an fp64 CPU conv of the same bf16
operands.

Error bar (derived, not measured).  Inputs and Q(w) are exact bf16 numbers and their products are
exact in fp32.  With ref = the fp64 conv of x and Q (+ bias), mag = the fp64 conv of |x| and |Q|
(+ |bias|) and k = (C/groups)*R*S:

    |y - ref| <= 2^-8 |ref| + (1 + 2^-8) (k + 3) 2^-23 mag        elementwise

2^-8 is bf16's unit roundoff (the output rounding); the second term allows one fp32 rounding or
truncation per accumulation step.  Q is _lib.restated_quantize(w.cpu(), bits, mode) in bf16, the
reference's own bf16 arithmetic on CPU.

Bit-exact cases use operands whose partial sums are exact in fp32 in any order (integer x in
[-4, 4]; weights that are multiples of 2^-7 with scale 1, or j/8), so y must equal ref.to(bf16):
this catches a wrong tap, a straddled row end or a wrong rounding.

The operands, the reference and the bar live in tests/_bf16_cases.py, shared with
tests/test_gpu_bf16_conv_paths.py (every kernel instance, staging and store path)."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from po2_quantization_amd import _lib
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.models.quantized_conv import QuantizedConv2d, _torch_epilogue
from po2_quantization_amd.utils.quantizers import NATIVE_MODES, quantizer_dict
from tests._bf16_cases import BF, BITS, MODES, assert_bar, exact_case, quantized, random_case, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N, C, H, W, K, R, stride, pad, dil)
SHAPES = [
    (2, 3, 9, 7, 10, 3, 1, 1, 1),        # stem-like C, odd W, odd H*W, K not a multiple of 16
    (1, 20, 11, 15, 24, 3, 2, 1, 1),     # stride 2, odd sizes, C not a multiple of 8
    (2, 72, 8, 10, 40, 3, 1, 1, 1),      # several channel chunks with a ragged last one
    (1, 40, 9, 9, 16, 1, 1, 0, 1),       # 1x1
    (1, 32, 7, 7, 32, 1, 2, 0, 1),       # 1x1 with stride 2 on odd rows
    (1, 8, 12, 13, 8, 5, 1, 2, 1),       # 5x5
    (2, 16, 10, 12, 16, 3, 1, 2, 2),     # dilation 2
    (1, 16, 5, 36, 16, 3, 1, 1, 1),      # 8-byte store path
    (2, 32, 6, 20, 64, 3, 1, 1, 1),      # 8-byte store path
    (3, 16, 1, 4, 16, 3, 1, 1, 1),       # one-row image
    (2, 16, 224, 224, 16, 3, 1, 1, 1),   # the bench geometry: many tiles
]
# depthwise (N, C, H, W, R, stride, pad), groups = C
DW_SHAPES = [(2, 24, 9, 9, 3, 1, 1), (1, 40, 10, 7, 3, 2, 1), (1, 8, 6, 6, 5, 1, 2)]


def native(x, w, b, stride, pad, dil, groups, mode):
    y = _lib.qconv2d_bf16(x.to(DEV), w.to(DEV), b.to(DEV) if b is not None else None, stride, pad, dil, groups, BITS,
                          mode)
    assert y.dtype == BF
    return y


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_error_bar(shape, mode, bias):
    N, C, H, W, K, R, st, pad, dil = shape
    x, w, b = random_case(shape, 1, 11, bias)
    ref, mag = reference(x, quantized(w, mode), b, st, pad, dil, 1)
    y = native(x, w, b, st, pad, dil, 1, mode)
    assert tuple(y.shape) == tuple(ref.shape)
    assert_bar(y, ref, mag, C * R * R, "%s %s" % (shape, mode))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_bit_exact(shape, mode, bias):
    N, C, H, W, K, R, st, pad, dil = shape
    x, w, b = exact_case(shape, 1, 12, bias, mode)
    q = quantized(w, mode)
    if mode != "none":
        assert bool((q.double() * 128 == (q.double() * 128).round()).all())  # the premise: multiples of 2^-7
    bd = b.double() if b is not None else None
    ref = F.conv2d(x.double(), q.double(), bd, st, pad, dil, 1).to(BF)
    y = native(x, w, b, st, pad, dil, 1, mode).cpu()
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), \
        "%d of %d elements differ" % (int((y != ref).sum()), y.numel())


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depthwise(shape, mode, bias):
    N, C, H, W, R, st, pad = shape
    full = (N, C, H, W, C, R)
    x, w, b = random_case(full, C, 13, bias)
    ref, mag = reference(x, quantized(w, mode), b, st, pad, 1, C)
    assert_bar(native(x, w, b, st, pad, 1, C, mode), ref, mag, R * R, "dw %s %s" % (shape, mode))
    x, w, b = exact_case(full, C, 14, bias, mode)
    bd = b.double() if b is not None else None
    ref = F.conv2d(x.double(), quantized(w, mode).double(), bd, st, pad, 1, C).to(BF)
    y = native(x, w, b, st, pad, 1, C, mode).cpu()
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16))


def test_weight_special_values():
    x = torch.randn(1, 16, 6, 8).to(BF)
    y = native(x, torch.zeros(16, 16, 3, 3, dtype=BF), None, 1, 1, 1, 1, "po2")
    assert bool(torch.isnan(y).all())  # scale 0: w / scale is NaN, as in the reference
    w = (torch.randn(16, 16, 3, 3) * 0.1).to(BF)
    w[3, 5, 1, 1] = float("nan")
    for mode in ("po2", "po2+"):
        assert bool(torch.isnan(native(x, w, None, 1, 1, 1, 1, mode)).all())


@pytest.mark.parametrize("where", [(4, 5), (0, 0), (7, 9)], ids=["interior", "corner", "last"])
def test_single_inf_in_x(where):
    shape = (1, 16, 8, 10, 16, 3, 1, 1, 1)
    x, w, b = random_case(shape, 1, 15, True)
    x[0, 7, where[0], where[1]] = float("inf")
    ref, _ = reference(x, quantized(w, "po2"), b, 1, 1, 1, 1)
    y = native(x, w, b, 1, 1, 1, 1, "po2").cpu()
    assert torch.equal(torch.isfinite(y.float()), torch.isfinite(ref))
    assert not bool(torch.isfinite(ref).all())


def test_errors():
    x = torch.randn(1, 16, 8, 8, device=DEV).to(BF)
    w = torch.randn(16, 16, 3, 3, device=DEV)
    with pytest.raises(_lib.Po2qError, match="bfloat16"):
        _lib.qconv2d_bf16(x, w, None, 1, 1)  # fp32 weight with a bf16 input
    mod = QuantizedConv2d(16, 16, 3, quantize_fn=quantizer_dict["po2"]).to(DEV)  # fp32 parameters
    with torch.no_grad(), pytest.raises(_lib.Po2qError, match="bfloat16"):
        mod(x)
    with pytest.raises(_lib.Po2qError, match="lin"):
        _lib.qconv2d_bf16(x, w.to(BF), None, 1, 1, mode="lin")
    with pytest.raises(_lib.Po2qError, match="groups"):
        _lib.qconv2d_bf16(x, w[:, :8].to(BF).contiguous(), None, 1, 1, groups=2)
    mod = mod.bfloat16()
    with pytest.raises(_lib.Po2qError, match="no_grad"):
        mod(x)  # the weight requires grad and grad mode is on
    with torch.no_grad():
        assert mod(x).dtype == BF
    lin = QuantizedConv2d(16, 16, 3, quantize_fn=quantizer_dict["lin"]).to(DEV).bfloat16()
    with torch.no_grad(), pytest.raises(_lib.Po2qError):
        lin(x)
    assert _lib.qconv2d_bf16(torch.empty(0, 16, 8, 8, device=DEV, dtype=BF), w.to(BF), None, 2, 1).shape == (0, 16, 4, 4)


def _capi_call(L, x, w, b, y, ws, geom, mode, ws_bytes=None):
    return L.po2q_qconv2d_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(),
                               *geom, BITS, 1, mode, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_capi_and_op_equal_lib_and_errors_leave_y_untouched():
    shape = (2, 20, 11, 15, 24, 3, 2, 1, 1)
    N, C, H, W, K, R, st, pad, dil = shape
    x, w, b = (t.to(DEV) for t in random_case(shape, 1, 16, True))
    want = _lib.qconv2d_bf16(x, w, b, st, pad, dil, 1, BITS, "po2+")
    geom = (N, C, H, W, K, R, R, st, st, pad, pad, dil, dil, 1)
    L = _lib.load()
    nbytes = L.po2q_qconv2d_bf16_workspace_bytes(*geom, BITS, 1, 2)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    y = torch.full_like(want, -7.0)
    sentinel = y.clone()
    assert _capi_call(L, x, w, b, y, ws, geom, 3) == 2            # lin: unsupported
    assert _capi_call(L, x, w, b, y, ws, geom, 2, ws_bytes=8) == 3  # short workspace
    bad = list(geom)
    bad[7] = 0
    assert _capi_call(L, x, w, b, y, ws, tuple(bad), 2) == 1 and b"stride" in L.po2q_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y, sentinel)
    assert _capi_call(L, x, w, b, y, ws, geom, 2) == 0
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))
    yo = torch.ops.po2q.qconv2d_bf16(x, w, b, [st, st], [pad, pad], [dil, dil], 1, BITS, 2, 1)
    assert yo.dtype == BF and torch.equal(yo.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("mode", ["po2", "po2+", None])
def test_module(mode):
    torch.manual_seed(17)
    qfn = quantizer_dict[mode] if mode else None
    mod = QuantizedConv2d(20, 24, 3, stride=1, padding=1, bias=True, quantize_fn=qfn, bits=BITS).bfloat16().to(DEV)
    bn = nn.BatchNorm2d(24)
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_()
        bn.bias.normal_()
    bn = bn.bfloat16().to(DEV).eval()
    x = torch.randn(2, 20, 9, 11).to(BF)
    res = torch.randn(2, 24, 9, 11).to(BF).to(DEV)
    with torch.no_grad():
        y = mod(x.to(DEV))
        fused = mod.fused(x.to(DEV), bn, "relu", res)
        seq = _torch_epilogue(y, bn, "relu", res)
        y3 = mod(x[0].to(DEV))  # unbatched input, as in the fp32 path
    assert y.dtype == BF and fused.dtype == BF
    w, b = mod.weight.detach().cpu(), mod.bias.detach().cpu()
    ref, mag = reference(x, quantized(w, mode or "none"), b, 1, 1, 1, 1)
    assert_bar(y, ref, mag, 20 * 9, "module %s" % mode)
    assert torch.equal(fused.view(torch.int16), seq.view(torch.int16))
    assert y3.dim() == 3 and torch.equal(y3.view(torch.int16), y[0].view(torch.int16))


@pytest.mark.parametrize("name", ["resnet20", "mobilenet"])
def test_model_layers(name):
    """Every conv of an eval bf16 forward meets the bar against its own fp64 conv (no whole-model
    tolerance: the layers' roundings compound in a way that cannot be derived)."""
    torch.manual_seed(18)
    model = get_model(name, 10, quantizer_dict["po2"], BITS, (32, 32)).eval().bfloat16().to(DEV)
    rec = []
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    for m in convs:
        m.register_forward_hook(lambda mod, inp, out: rec.append((mod, inp[0].detach().cpu(), out.detach().cpu())))
    x = torch.randn(2, 3, 32, 32).to(BF).to(DEV)
    with torch.no_grad():
        logits = model(x)
    assert logits.dtype == BF and tuple(logits.shape) == (2, 10) and bool(torch.isfinite(logits.float()).all())
    assert {id(m) for m, _, _ in rec} == {id(m) for m in convs}  # every conv ran, through the hooks
    for m, xi, yo in rec:
        w = m.weight.detach().cpu()
        mode = NATIVE_MODES.get(getattr(m, "quantize_fn", None))
        q = _lib.restated_quantize(w, m.bits, mode) if mode else w
        b = m.bias.detach().cpu() if m.bias is not None else None
        ref, mag = reference(xi, q, b, m.stride, m.padding, m.dilation, m.groups)
        k = (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1]
        assert yo.dtype == BF
        assert_bar(yo, ref, mag, k, "%s %s" % (name, tuple(w.shape)))
