"""GPU: every conv_bf16x1<CC, NT, NJ> instance, staging path and store path of the native bf16 conv
forward (po2q_qconv2d_bf16), and its depthwise kernel, at the shapes of tests/_bf16_cases.py
(tests/test_bf16_conv_cpu.py pins which kernel each of them runs).

Reference and bar are those of tests/test_gpu_bf16_conv.py: the fp64 CPU conv of the same bf16
operands, |y - ref| <= 2^-8 |ref| + (1 + 2^-8) (k + 3) 2^-23 mag elementwise, and bit-for-bit
equality on operands whose partial sums are exact in fp32 in any order.  Premise of the exact runs:
x is an integer in [-4, 4] and Q a multiple of 2^-7 (or j/8) of magnitude <= 1, so every partial sum
is a multiple of 2^-7 below 4 k, k = C*R*S; 4 k 128 < 2^24 keeps it exact.  No other tolerance is
used here: staging width, store width and pointer alignment move data and never change arithmetic,
so runs that differ only in those are compared for equality.

Every conv of this file goes through the C ABI with y placed inside a larger buffer of sentinel
values, at least 64 elements on either side; both bands must come back untouched."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from po2_quantization_amd import _lib
from tests import _bf16_cases as cases
from tests._bf16_cases import BF, BITS, MODES, assert_bar, bar, exact_case, quantized, random_case, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # bf16 elements on either side of y (128 bytes: y itself starts 8-byte aligned)
SENTINEL = 0x5a5a   # a finite bf16 pattern no case produces across a whole band
MODE_ID = {"none": 0, "po2": 1, "po2+": 2}
BIAS = pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])


def _bits(t):
    return t.contiguous().view(torch.int16)


def run(x, w, b, shape, groups, mode, bits=BITS, fsr=1, y_shift=0, refused=False):
    """po2q_qconv2d_bf16 through the C ABI on device tensors as they are (their data pointers reach the
    kernels unchanged); y starts y_shift elements past an 8-byte aligned address inside a guard buffer.
    Returns y on the CPU after checking the status and both guard bands; a call that must be refused
    (refused=True) has to leave y untouched as well."""
    L = _lib.load()
    P, Q = cases.out_size(shape)
    n = shape[0] * shape[4] * P * Q
    geom = cases.geom14(shape, groups)
    nbytes = L.po2q_qconv2d_bf16_workspace_bytes(*geom, bits, fsr, MODE_ID[mode])
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    buf = torch.full((GUARD + 4 + n + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 8 == 0
    y = buf[GUARD + y_shift:GUARD + y_shift + n]
    for t in (x, w) + ((b,) if b is not None else ()):
        assert t.is_contiguous() and t.dtype == BF and t.is_cuda
    st = L.po2q_qconv2d_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), *geom,
                             bits, fsr, MODE_ID[mode], ws.data_ptr(), ws.numel(),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (st != 0) == refused, (st, L.po2q_last_error())
    out = buf.cpu()
    lo, hi = out[:GUARD + y_shift], out[GUARD + y_shift + n:]
    assert bool((lo == SENTINEL).all()), "%d elements written before y" % int((lo != SENTINEL).sum())
    assert bool((hi == SENTINEL).all()), "%d elements written after y" % int((hi != SENTINEL).sum())
    body = out[GUARD + y_shift:GUARD + y_shift + n]
    if st != 0:
        assert bool((body == SENTINEL).all()), "a refused call wrote y"
        return None
    return body.view(BF).view(shape[0], shape[4], P, Q)


def dev(*ts):
    return tuple(t.to(DEV) if t is not None else None for t in ts)


def groups_of(shape, dw):
    return shape[1] if dw else 1


@functools.lru_cache(maxsize=None)
def random_ref(shape, dw, mode, bias):
    """(x, w, b, ref, mag) of a case, computed once and shared; nothing changes them afterwards."""
    g = groups_of(shape, dw)
    x, w, b = random_case(shape, g, 21, bias)
    ref, mag = reference(x, quantized(w, mode), b, *cases.conv_args(shape), g)
    return x, w, b, ref, mag


def check_bar(shape, dw, mode, bias):
    g = groups_of(shape, dw)
    x, w, b, ref, mag = random_ref(shape, dw, mode, bias)
    y = run(*dev(x, w, b), shape, g, mode)
    assert tuple(y.shape) == tuple(ref.shape)
    assert_bar(y, ref, mag, (shape[1] // g) * shape[5] * shape[6], "%s %s" % (shape, mode))


def check_exact(shape, dw, mode, bias):
    g = groups_of(shape, dw)
    k = (shape[1] // g) * shape[5] * shape[6]
    assert 4 * k * 128 < 2 ** 24  # the premise: every partial sum is exact in fp32
    x, w, b = exact_case(shape, g, 22, bias, mode)
    q = quantized(w, mode)
    if mode != "none":
        assert bool((q.double() * 128 == (q.double() * 128).round()).all())  # the premise: multiples of 2^-7
    bd = b.double() if b is not None else None
    ref = F.conv2d(x.double(), q.double(), bd, *cases.conv_args(shape), g).to(BF)
    y = run(*dev(x, w, b), shape, g, mode)
    assert torch.equal(_bits(y), _bits(ref)), "%d of %d elements differ" % (int((y != ref).sum()), y.numel())


# ---- every instance and edge: error bar and bit-exact -----------------------------------------------
@BIAS
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", cases.DENSE, ids=cases.case_id)
def test_dense_error_bar(shape, mode, bias):
    check_bar(shape, False, mode, bias)


@BIAS
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", cases.DENSE, ids=cases.case_id)
def test_dense_bit_exact(shape, mode, bias):
    check_exact(shape, False, mode, bias)


@BIAS
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", cases.DEPTHWISE, ids=cases.case_id)
def test_depthwise_error_bar(shape, mode, bias):
    check_bar(shape, True, mode, bias)


@BIAS
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", cases.DEPTHWISE, ids=cases.case_id)
def test_depthwise_bit_exact(shape, mode, bias):
    check_exact(shape, True, mode, bias)


# ---- pointer alignment: 2-byte aligned x, w, bias and y ---------------------------------------------
def displaced(t):
    """The same values one bf16 element past an aligned address: 2-byte but not 4-byte aligned, and
    contiguous, so nothing on the way to the kernel copies it."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 4 == 2
    return v


@pytest.mark.parametrize("which", ["x", "w", "bias", "y", "all"])
@pytest.mark.parametrize("mode", ["po2", "none"])
@pytest.mark.parametrize("shape", cases.ALIGNMENT, ids=cases.case_id)
def test_two_byte_aligned_pointers(shape, mode, which):
    x, w, b, ref, mag = random_ref(shape, False, mode, True)
    x, w, b = dev(x, w, b)
    for t in (x, w, b):
        assert t.data_ptr() % 8 == 0
    want = run(x, w, b, shape, 1, mode)
    assert_bar(want, ref, mag, shape[1] * shape[5] * shape[6], "%s aligned" % (shape,))
    xs, ws, bs = (displaced(t) if which in (name, "all") else t for t, name in ((x, "x"), (w, "w"), (b, "bias")))
    got = run(xs, ws, bs, shape, 1, mode, y_shift=1 if which in ("y", "all") else 0)
    assert torch.equal(_bits(got), _bits(want)), "%d of %d elements differ" % (int((got != want).sum()), got.numel())


@pytest.mark.parametrize("shape", cases.ALIGNMENT, ids=cases.case_id)
def test_channels_last_and_strided_inputs(shape):
    x, w, b, ref, mag = random_ref(shape, False, "po2", True)
    x, w, b = dev(x, w, b)
    stride, pad, dil = cases.conv_args(shape)
    want = run(x, w, b, shape, 1, "po2")
    y = _lib.qconv2d_bf16(x, w, b, stride, pad, dil, 1, BITS, "po2").cpu()  # the wrapper runs what the C ABI runs
    assert torch.equal(_bits(y), _bits(want))
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    y = _lib.qconv2d_bf16(cl, w, b, stride, pad, dil, 1, BITS, "po2").cpu()
    assert torch.equal(_bits(y), _bits(want))
    wide = torch.zeros(shape[0], shape[1] + 3, shape[2] + 2, shape[3] + 5, dtype=BF, device=DEV)
    sl = wide[:, 2:2 + shape[1], 1:1 + shape[2], 3:3 + shape[3]]
    sl.copy_(x)
    assert not sl.is_contiguous()
    wwide = torch.zeros(shape[4], shape[1] * 2, shape[5], shape[6], dtype=BF, device=DEV)
    wsl = wwide[:, ::2]
    wsl.copy_(w)
    y = _lib.qconv2d_bf16(sl, wsl, b, stride, pad, dil, 1, BITS, "po2").cpu()
    assert torch.equal(_bits(y), _bits(want))


# ---- the conv's quantize-and-pack equals the native quantizer ---------------------------------------
QUANT_SHAPES = [((2, 40, 6, 10, 80, 3, 3, 1, 1, 1, 1, 1, 1), False),   # 2 k-blocks x 3 chunks
                (cases.DEPTHWISE[0], True)]
QUANT_WINDOWS = [(2, 1), (3, 1), (5, 1), (8, 1), (4, 2)]  # (bits, fsr)


@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("bits,fsr", QUANT_WINDOWS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape,dw", QUANT_SHAPES, ids=["dense", "depthwise"])
def test_quantize_and_pack_equals_the_native_quantizer(shape, dw, bits, fsr, mode):
    g = groups_of(shape, dw)
    if not dw:
        p = cases.parse_plan(cases.describe(shape))
        assert p.kblocks > 1 and p.chunks > 1
    x, w, b = random_case(shape, g, 23, True)  # w = randn * 0.1: every Q(w) is a normal bf16
    q_cpu = _lib.restated_quantize(w, bits, mode, fsr)
    assert bool((q_cpu.float().abs() >= 2.0 ** -126).all())
    xd, wd, bd = dev(x, w, b)
    qd = _lib.quantize(wd, bits, mode, fsr)
    assert qd.dtype == BF and torch.equal(_bits(qd.cpu()), _bits(q_cpu))
    fused = run(xd, wd, bd, shape, g, mode, bits, fsr)
    two_step = run(xd, qd.contiguous(), bd, shape, g, "none")
    assert torch.equal(_bits(fused), _bits(two_step)), "%d elements differ" % int((fused != two_step).sum())
    stride, pad, dil = cases.conv_args(shape)
    wrapped = _lib.qconv2d_bf16(xd, wd, bd, stride, pad, dil, g, bits, mode, fsr).cpu()
    assert torch.equal(_bits(wrapped), _bits(fused))
    ref, mag = reference(x, q_cpu, b, stride, pad, dil, g)
    k = (shape[1] // g) * shape[5] * shape[6]
    assert_bar(fused, ref, mag, k, "%s bits %d fsr %d %s" % (shape, bits, fsr, mode))


# ---- non-finite activations -------------------------------------------------------------------------
NONFINITE_SHAPES = [((2, 16, 9, 70, 16, 3, 3, 1, 1, 1, 1, 1, 1), False),   # pair staging, several tiles
                    ((2, 16, 9, 71, 16, 3, 3, 1, 1, 1, 1, 1, 1), False),   # odd W
                    (cases.DEPTHWISE[0], True)]
INF, NAN = float("inf"), float("nan")


def kind(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    t = t.double()
    return torch.isposinf(t) * 1 + torch.isneginf(t) * 2 + torch.isnan(t) * 3


def places(shape, dw):
    H, W = shape[2], shape[3]
    # dense: the last column of the first Q tile (stride 1, pad 1: output column = input column);
    # the depthwise kernel has no tiles: the column before the last
    tq = W - 1 if dw else cases.parse_plan(cases.describe(shape)).TQ
    assert tq < W
    return {"interior": (H // 2, W // 2), "corner": (0, 0), "last": (H - 1, W - 1), "tile_edge": (1, tq - 1)}


def check_nonfinite(shape, dw, x, w, b):
    g = groups_of(shape, dw)
    ref, mag = reference(x, quantized(w, "po2"), b, *cases.conv_args(shape), g)
    y = run(*dev(x, w, b), shape, g, "po2")
    assert torch.equal(kind(y), kind(ref)), "NaN / inf pattern: %d elements differ" % int((kind(y) != kind(ref)).sum())
    fin = torch.isfinite(ref)
    assert not bool(fin.all()) and bool(fin.any())
    # finite outputs: the bar, with mag taken over the finite inputs they depend on (a non-finite input
    # reaches no finite output: every Q(w) is nonzero)
    xf = torch.where(torch.isfinite(x.float()), x.float(), torch.zeros(())).to(BF)
    reff, magf = reference(xf, quantized(w, "po2"), b, *cases.conv_args(shape), g)
    assert torch.equal(reff[fin], ref[fin])
    err = (y.double() - ref).abs()[fin]
    assert bool((err <= bar(reff, magf, (shape[1] // g) * shape[5] * shape[6])[fin]).all())


@pytest.mark.parametrize("value", [INF, -INF, NAN], ids=["pinf", "ninf", "nan"])
@pytest.mark.parametrize("where", ["interior", "corner", "last", "tile_edge"])
@pytest.mark.parametrize("shape,dw", NONFINITE_SHAPES, ids=["pair", "oddW", "depthwise"])
def test_one_nonfinite_activation(shape, dw, where, value):
    x, w, b = random_case(shape, groups_of(shape, dw), 24, True)
    assert bool((quantized(w, "po2") != 0).all())
    h, wc = places(shape, dw)[where]
    x = x.clone()
    x[shape[0] - 1, 5, h, wc] = value
    check_nonfinite(shape, dw, x, w, b)


@pytest.mark.parametrize("shape,dw", NONFINITE_SHAPES, ids=["pair", "oddW", "depthwise"])
def test_nonfinite_activations_together(shape, dw):
    """+inf, -inf and NaN in one input, +inf and -inf close enough to meet in one output (NaN there)."""
    x, w, b = random_case(shape, groups_of(shape, dw), 25, True)
    pl = places(shape, dw)
    x = x.clone()
    x[0, 5, pl["interior"][0], pl["interior"][1]] = INF
    x[0, 5, pl["interior"][0], pl["interior"][1] + 1] = -INF
    x[0, 2, 0, 0] = -INF
    x[shape[0] - 1, 7, pl["last"][0], pl["last"][1]] = NAN
    x[shape[0] - 1, 3, pl["tile_edge"][0], pl["tile_edge"][1]] = INF
    check_nonfinite(shape, dw, x, w, b)


# ---- kernels that do not fit LDS --------------------------------------------------------------------
def test_too_large_kernel_is_an_error_and_leaves_y_untouched():
    shape = cases.TOO_LARGE
    x, w, b = dev(*random_case(shape, 1, 26, True))
    with pytest.raises(_lib.Po2qError, match="LDS"):
        _lib.qconv2d_bf16(x, w, b, *cases.conv_args(shape), 1, BITS, "po2")
    assert run(x, w, b, shape, 1, "po2", refused=True) is None  # non-zero status, y and both bands keep the sentinel
    assert b"LDS" in _lib.load().po2q_last_error()


def test_largest_kernel_that_fits_runs():
    assert cases.parse_lds(cases.describe(cases.LARGEST)) > 48 * 1024
    check_bar(cases.LARGEST, False, "po2", True)
