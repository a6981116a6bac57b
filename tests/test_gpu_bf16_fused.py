"""GPU: the fused bf16 conv entry (po2q_qconv2d_fused_bf16): eval BatchNorm affine, residual add and
activation in the store epilogue of conv_bf16x1 / conv_dw_b16, at every shape of tests/_bf16_cases.py
(all 18 instances, both staging paths, both store paths, the depthwise kernel).

Contract (include/po2q.h), per output, acc the fp32 accumulator of po2q_qconv2d_bf16:
    v = acc + bias[k];  v = v * s[k] + t[k];  v = v + r[n, k, p, q];  y = bf16_rne(act(v))
with one rounding to bf16, at the end.

Error bar (derived, not measured).  c and mag are what reference() returns (the fp64 conv with bias
and the same conv of the absolute values); s, t, r are the fp32 / bf16 arguments as doubles (an
absent scale is 1, an absent shift or residual 0); k = (C / groups) R S; ref = act64(c s + t + r):
    E   = |s| (k + 3) 2^-23 mag + 2^-22 (|c s| + |t| + |r|)
    bar = 2^-8 |ref| + (1 + 2^-8) L E  [+ 2^-20 |ref| for silu]
  * |s| (k + 3) 2^-23 mag is the accumulation bound of the plain entry's bar (k additions and the bias
    add, each within 2^-24 of a partial sum bounded by mag), carried through the multiplication by s;
  * 2^-22 (|c s| + |t| + |r|) allows the three fp32 roundings of the multiply, the shift add and the
    residual add (each 2^-24 of a value bounded by the sum of the magnitudes; fused or not);
  * L is the activation's Lipschitz constant: 1 for none / relu / relu6, 1.1 for silu (its slope stays
    below 1.1); silu's expf and division add a few fp32 ulps, 2^-20 |ref|;
  * 2^-8 |ref| (and the factor 1 + 2^-8 on the rest) is the final rounding to bf16.

Bit-exact cases.  x, w, bias from exact_case (integers in [-4, 4], Q(w) and bias multiples of 2^-7 /
2^-3), s in {0.5, 1, 2, -1, 0.25, -2}, t = j / 8 with |j| <= 8, r = j / 8 with |j| <= 32: acc + bias,
v s + t and + r are all multiples of 2^-9 below 2^15, exact in fp32 in any summation order and with or
without FMA contraction, so y must equal bf16_rne of the fp64 result bit for bit.  That catches a
residual read at the wrong pixel or channel, post_scale[lane & 15] without the k-block offset, an
activation applied before the add, and a double rounding.

Every C ABI call places y inside a buffer of sentinel values, 64 elements on either side; both
bands must come back untouched, and a refused call leaves y itself untouched."""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from po2_quantization_amd import _lib
from po2_quantization_amd.models import quantized_conv as qc
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.models.quantized_conv import QuantizedConv2d, _torch_epilogue
from po2_quantization_amd.utils.quantizers import quantizer_dict
from tests import _bf16_cases as cases
from tests._bf16_cases import BF, BITS, exact_case, quantized, random_case, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = 0x5a5a
MODE_ID = {"none": 0, "po2": 1, "po2+": 2, "lin": 3}
ACT_ID = {"none": 0, "relu": 1, "relu6": 2, "silu": 3}

ALL = [(s, False) for s in cases.DENSE] + [(s, True) for s in cases.DEPTHWISE]
ALL_IDS = [("dw-" if dw else "") + cases.case_id(s) for s, dw in ALL]
# (post_scale, post_shift, residual, act)
TABLE = [(True, True, False, "relu"), (True, True, True, "relu"), (False, False, True, "none"),
         (True, False, False, "relu6"), (False, True, True, "silu"), (False, False, False, "relu")]
WORST = {}


def _bits(t):
    return t.contiguous().view(torch.int16)


def dev(*ts):
    return tuple(t.to(DEV) if t is not None else None for t in ts)


def groups_of(shape, dw):
    return shape[1] if dw else 1


def _ptr(t):
    return t.data_ptr() if t is not None else None


def run(x, w, b, shape, groups, mode, ps=None, pb=None, res=None, act=0, y_shift=0, refused=False, ws_cut=0,
        plain=False):
    """po2q_qconv2d_fused_bf16 (plain: po2q_qconv2d_bf16) through the C ABI on device tensors as they are;
    y starts y_shift elements past an 8-byte aligned address inside a guard buffer.  Returns y on the CPU
    after checking the status and both guard bands; a refused call has to leave y untouched as well."""
    L = _lib.load()
    P, Q = cases.out_size(shape)
    n = shape[0] * shape[4] * P * Q
    geom = cases.geom14(shape, groups)
    mode_id = MODE_ID[mode]
    nbytes = L.po2q_qconv2d_bf16_workspace_bytes(*geom, BITS, 1, mode_id)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    buf = torch.full((GUARD + 4 + n + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 8 == 0
    y = buf[GUARD + y_shift:GUARD + y_shift + n]
    for t in (x, w, b, res):
        assert t is None or (t.is_contiguous() and t.dtype == BF and t.is_cuda)
    for t in (ps, pb):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda and t.numel() == shape[4])
    assert res is None or res.numel() == n
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wsb = nbytes - ws_cut if ws_cut else ws.numel()
    if plain:
        st = L.po2q_qconv2d_bf16(x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), *geom, BITS, 1, mode_id,
                                 ws.data_ptr(), wsb, stream)
    else:
        st = L.po2q_qconv2d_fused_bf16(x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), *geom, BITS, 1, mode_id,
                                       _ptr(ps), _ptr(pb), _ptr(res), act, ws.data_ptr(), wsb, stream)
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


# ---- reference and bar ------------------------------------------------------------------------------
def act64(v, act):
    if act == "relu":
        return v.clamp_min(0)
    if act == "relu6":
        return v.clamp(0, 6)
    if act == "silu":
        return v * torch.sigmoid(v)
    return v


def fused_ref_bar(c, mag, k, s, t, r, act):
    """(ref, bar) of the docstring; s, t [K] or None, r like c or None, all taken as doubles."""
    sd = s.double().view(1, -1, 1, 1) if s is not None else torch.ones(1, 1, 1, 1, dtype=torch.float64)
    td = t.double().view(1, -1, 1, 1) if t is not None else torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    rd = r.double() if r is not None else torch.zeros_like(c)
    ref = act64(c * sd + td + rd, act)
    E = sd.abs() * (k + 3) * 2.0 ** -23 * mag + 2.0 ** -22 * ((c * sd).abs() + td.abs() + rd.abs())
    lip = 1.1 if act == "silu" else 1.0
    tol = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * lip * E
    if act == "silu":
        tol = tol + 2.0 ** -20 * ref.abs()
    return ref, tol


def assert_fused_bar(y, c, mag, k, s, t, r, act, group, what=""):
    ref, tol = fused_ref_bar(c, mag, k, s, t, r, act)
    err = (y.double().cpu() - ref).abs()
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print("%s %s worst |y - ref| / bar = %.3f (group %s so far %.3f)" % (what, act, ratio, group, WORST[group]))
    assert y.dtype == BF and tuple(y.shape) == tuple(ref.shape)
    assert torch.isfinite(y.float()).all(), what
    assert bool((err <= tol).all()), (what, ratio)


@functools.lru_cache(maxsize=None)
def random_ref(shape, dw, mode, bias):
    """(x, w, b, c, mag, s, t, r) of a case, computed once and shared; nothing changes them afterwards."""
    g = groups_of(shape, dw)
    x, w, b = random_case(shape, g, 31, bias)
    c, mag = reference(x, quantized(w, mode), b, *cases.conv_args(shape), g)
    gen = torch.Generator().manual_seed(32)
    s = torch.randn(shape[4], generator=gen)
    t = torch.randn(shape[4], generator=gen)
    r = torch.randn(c.shape, generator=gen).to(BF)
    return x, w, b, c, mag, s, t, r


def check_bar(shape, dw, mode, bias, row, group):
    has_s, has_t, has_r, act = row
    g = groups_of(shape, dw)
    x, w, b, c, mag, s, t, r = random_ref(shape, dw, mode, bias)
    s, t, r = (s if has_s else None), (t if has_t else None), (r if has_r else None)
    y = run(*dev(x, w, b), shape, g, mode, *dev(s, t, r), ACT_ID[act])
    assert_fused_bar(y, c, mag, (shape[1] // g) * shape[5] * shape[6], s, t, r, act, group, "%s %s" % (shape, mode))


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%d%d%d-%s" % (r[0], r[1], r[2], r[3]))
@pytest.mark.parametrize("shape,dw", ALL, ids=ALL_IDS)
def test_epilogue_table_error_bar(shape, dw, row):
    check_bar(shape, dw, "po2", True, row, "table")


@pytest.mark.parametrize("mode,bias", [("po2+", True), ("none", True), ("po2", False)],
                         ids=["po2plus", "none", "nobias"])
@pytest.mark.parametrize("shape,dw", ALL, ids=ALL_IDS)
def test_full_epilogue_other_modes_error_bar(shape, dw, mode, bias):
    check_bar(shape, dw, mode, bias, TABLE[1], "modes")


# ---- bit-exact --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [(True, True, True, "relu"), (False, False, True, "none"), (True, True, True, "relu6")],
                         ids=["111-relu", "001-none", "111-relu6"])
@pytest.mark.parametrize("shape,dw", ALL, ids=ALL_IDS)
def test_bit_exact(shape, dw, row):
    has_s, has_t, has_r, act = row
    g = groups_of(shape, dw)
    K = shape[4]
    x, w, b = exact_case(shape, g, 33, True, "po2")
    q = quantized(w, "po2")
    assert bool((q.double() * 128 == (q.double() * 128).round()).all())  # the premise: multiples of 2^-7
    c, mag = reference(x, q, b, *cases.conv_args(shape), g)
    gen = torch.Generator().manual_seed(34)
    s = torch.tensor([0.5, 1.0, 2.0, -1.0, 0.25, -2.0])[torch.randint(0, 6, (K,), generator=gen)] if has_s else None
    t = torch.randint(-8, 9, (K,), generator=gen).float() / 8 if has_t else None
    r = (torch.randint(-32, 33, c.shape, generator=gen).float() / 8).to(BF) if has_r else None
    sd = s.double().view(1, -1, 1, 1) if has_s else 1.0
    td = t.double().view(1, -1, 1, 1) if has_t else 0.0
    rd = r.double() if has_r else 0.0
    pre = c * sd + td + rd
    # the premise: every intermediate is a multiple of 2^-9 and, times 2^9, below 2^24 (mag bounds every
    # partial sum of the accumulation, 2 mag + 1 + 4 every later value)
    assert bool((pre * 512 == (pre * 512).round()).all()) and float((2 * mag + 5).max()) * 512 < 2 ** 24
    ref = act64(pre, act).to(BF)
    y = run(*dev(x, w, b), shape, g, "po2", *dev(s, t, r), ACT_ID[act])
    assert torch.equal(_bits(y), _bits(ref)), "%d of %d elements differ" % (int((y != ref).sum()), y.numel())


# ---- identity: nothing to fuse gives the plain entry's bits -------------------------------------------
@pytest.mark.parametrize("shape,dw", ALL, ids=ALL_IDS)
def test_identity_equals_the_plain_entry(shape, dw):
    g = groups_of(shape, dw)
    x, w, b = dev(*random_ref(shape, dw, "po2", True)[:3])
    want = run(x, w, b, shape, g, "po2", plain=True)
    got = run(x, w, b, shape, g, "po2")
    assert torch.equal(_bits(got), _bits(want))


# ---- alignment ----------------------------------------------------------------------------------------
def displaced(t):
    """The same values one element past an aligned address, contiguous."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % (2 * t.element_size()) == t.element_size()
    return v


@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("shape", cases.ALIGNMENT, ids=cases.case_id)
def test_two_byte_aligned_residual_and_y(shape, act):
    x, w, b, c, mag, s, t, r = random_ref(shape, False, "po2", True)
    x, w, b, s, t, r = dev(x, w, b, s, t, r)
    assert r.data_ptr() % 8 == 0
    a = ACT_ID[act]
    want = run(x, w, b, shape, 1, "po2", s, t, r, a)
    assert_fused_bar(want, c, mag, shape[1] * shape[5] * shape[6], s.cpu(), t.cpu(), r.cpu(), act, "alignment")
    got = run(x, w, b, shape, 1, "po2", s, t, displaced(r), a)            # residual 2-byte aligned, y aligned
    assert torch.equal(_bits(got), _bits(want)), "%d elements differ" % int((got != want).sum())
    got = run(x, w, b, shape, 1, "po2", s, t, r, a, y_shift=1)            # y 2-byte aligned, residual aligned
    assert torch.equal(_bits(got), _bits(want)), "%d elements differ" % int((got != want).sum())
    got = run(x, w, b, shape, 1, "po2", s, t, displaced(r), a, y_shift=1)  # both
    assert torch.equal(_bits(got), _bits(want)), "%d elements differ" % int((got != want).sum())
    # post_scale / post_shift from the middle of a larger fp32 buffer (4-byte aligned only)
    got = run(x, w, b, shape, 1, "po2", displaced(s), displaced(t), r, a)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("shape", cases.ALIGNMENT, ids=cases.case_id)
def test_op_and_wrapper_equal_the_c_abi_on_any_layout(shape):
    x, w, b, c, mag, s, t, r = random_ref(shape, False, "po2", True)
    x, w, b, s, t, r = dev(x, w, b, s, t, r)
    stride, pad, dil = cases.conv_args(shape)
    want = run(x, w, b, shape, 1, "po2", s, t, r, 1)
    y = _lib.qconv2d_fused_bf16(x, w, b, stride, pad, dil, 1, BITS, "po2", 1, post_scale=s, post_shift=t, residual=r,
                                act="relu")
    assert y.dtype == BF and torch.equal(_bits(y.cpu()), _bits(want))
    op = torch.ops.po2q.qconv2d_fused_bf16

    def call(xi, ri):
        return op(xi, w, b, list(stride), list(pad), list(dil), 1, BITS, 1, 1, s, t, ri, 1).cpu()

    assert torch.equal(_bits(call(x, r)), _bits(want))
    xcl, rcl = x.contiguous(memory_format=torch.channels_last), r.contiguous(memory_format=torch.channels_last)
    assert not xcl.is_contiguous() and not rcl.is_contiguous()
    assert torch.equal(_bits(call(xcl, rcl)), _bits(want))
    wide = torch.zeros(shape[0], shape[1] + 3, shape[2] + 2, shape[3] + 5, dtype=BF, device=DEV)
    xs = wide[:, 2:2 + shape[1], 1:1 + shape[2], 3:3 + shape[3]]
    xs.copy_(x)
    rwide = torch.zeros(r.shape[0], r.shape[1], r.shape[2] + 1, r.shape[3] * 2, dtype=BF, device=DEV)
    rs = rwide[:, :, 1:, ::2]
    rs.copy_(r)
    assert not xs.is_contiguous() and not rs.is_contiguous()
    assert torch.equal(_bits(call(xs, rs)), _bits(want))


# ---- non-finite ---------------------------------------------------------------------------------------
NONFINITE = [(cases.ALIGNMENT[0], False), (cases.ALIGNMENT[2], False), (cases.DEPTHWISE[0], True)]
NONFINITE_IDS = ["vec-store", "2byte-store", "depthwise"]


@pytest.mark.parametrize("shape,dw", NONFINITE, ids=NONFINITE_IDS)
def test_nan_shift_poisons_exactly_its_channel(shape, dw):
    g = groups_of(shape, dw)
    x, w, b, c, mag, s, t, r = random_ref(shape, dw, "po2", True)
    kk = shape[4] - 3
    t = t.clone()
    t[kk] = float("nan")
    y = run(*dev(x, w, b), shape, g, "po2", *dev(s, t, r), ACT_ID["relu"])
    nan = torch.isnan(y.float())
    want = torch.zeros_like(nan)
    want[:, kk] = True
    assert torch.equal(nan, want)


@pytest.mark.parametrize("shape,dw", NONFINITE, ids=NONFINITE_IDS)
def test_infinite_residual_under_relu6(shape, dw):
    g = groups_of(shape, dw)
    x, w, b, c, mag, s, t, r = random_ref(shape, dw, "po2", True)
    r = r.clone()
    P, Q = cases.out_size(shape)
    hi, lo = (shape[0] - 1, shape[4] - 1, P - 1, Q - 1), (0, 1, P // 2, 0)
    r[hi] = float("inf")
    r[lo] = float("-inf")
    y = run(*dev(x, w, b), shape, g, "po2", *dev(s, t, r), ACT_ID["relu6"])
    assert float(y[hi]) == 6.0 and float(y[lo]) == 0.0
    rf = torch.where(torch.isfinite(r.float()), r.float(), torch.zeros(())).to(BF)
    ref, tol = fused_ref_bar(c, mag, (shape[1] // g) * shape[5] * shape[6], s, t, rf, "relu6")
    ok = (y.double() - ref).abs() <= tol
    ok[hi] = ok[lo] = True
    assert bool(ok.all()) and bool(torch.isfinite(y.float()).all())


@pytest.mark.parametrize("act", ["relu", "relu6"])
@pytest.mark.parametrize("shape,dw", NONFINITE, ids=NONFINITE_IDS)
def test_nan_quantized_weight_stays_nan(shape, dw, act):
    g = groups_of(shape, dw)
    x, w, b, c, mag, s, t, r = random_ref(shape, dw, "po2", True)
    w0 = torch.zeros_like(w)  # max|w| = 0: Q(w) = NaN, as the reference quantizer gives
    assert bool(torch.isnan(quantized(w0, "po2").float()).all())
    y = run(*dev(x, w0, b), shape, g, "po2", *dev(s, t, r), ACT_ID[act])
    assert bool(torch.isnan(y.float()).all())


# ---- errors: rejected before any launch, y untouched ----------------------------------------------------
ERR_SHAPE = cases.ALIGNMENT[0]


def _err_args():
    x, w, b, c, mag, s, t, r = random_ref(ERR_SHAPE, False, "po2", True)
    return dev(x, w, b, s, t, r)


@pytest.mark.parametrize("act", [4, -1])
def test_unknown_activation_is_refused(act):
    x, w, b, s, t, r = _err_args()
    assert run(x, w, b, ERR_SHAPE, 1, "po2", s, t, r, act, refused=True) is None
    assert b"unknown activation" in _lib.load().po2q_last_error()


def test_lin_mode_is_refused():
    x, w, b, s, t, r = _err_args()
    assert run(x, w, b, ERR_SHAPE, 1, "lin", s, t, r, 1, refused=True) is None
    assert b"lin" in _lib.load().po2q_last_error()


def test_groups_2_is_refused():
    x, w, b, s, t, r = _err_args()
    w2 = w[:, :ERR_SHAPE[1] // 2].contiguous()
    assert run(x, w2, b, ERR_SHAPE, 2, "po2", s, t, r, 1, refused=True) is None
    assert b"groups" in _lib.load().po2q_last_error()


def test_too_large_kernel_is_refused():
    shape = cases.TOO_LARGE
    x, w, b = dev(*random_case(shape, 1, 35, True))
    P, Q = cases.out_size(shape)
    r = torch.zeros(shape[0], shape[4], P, Q, dtype=BF, device=DEV)
    assert run(x, w, b, shape, 1, "po2", None, None, r, 1, refused=True) is None
    assert b"LDS" in _lib.load().po2q_last_error()
    with pytest.raises(_lib.Po2qError, match="LDS"):
        _lib.qconv2d_fused_bf16(x, w, b, *cases.conv_args(shape), 1, BITS, "po2", 1, residual=r, act="relu")


def test_short_workspace_is_refused():
    x, w, b, s, t, r = _err_args()
    assert run(x, w, b, ERR_SHAPE, 1, "po2", s, t, r, 1, refused=True, ws_cut=1) is None
    assert b"workspace" in _lib.load().po2q_last_error()


def test_op_rejects_bad_epilogue_arguments():
    x, w, b, s, t, r = _err_args()
    stride, pad, dil = (list(v) for v in cases.conv_args(ERR_SHAPE))
    op = torch.ops.po2q.qconv2d_fused_bf16
    with pytest.raises(RuntimeError, match="residual"):
        op(x, w, b, stride, pad, dil, 1, BITS, 1, 1, s, t, r.float(), 1)
    with pytest.raises(RuntimeError, match="post_scale"):
        op(x, w, b, stride, pad, dil, 1, BITS, 1, 1, s.to(BF), t, r, 1)
    with pytest.raises(RuntimeError, match="residual"):
        op(x, w, b, stride, pad, dil, 1, BITS, 1, 1, s, t, r[:, :, :-1].contiguous(), 1)
    with pytest.raises(RuntimeError, match="post_scale"):
        op(x, w, b, stride, pad, dil, 1, BITS, 1, 1, s[:-1].contiguous(), t, r, 1)
    with pytest.raises(RuntimeError, match="unknown activation"):
        op(x, w, b, stride, pad, dil, 1, BITS, 1, 1, s, t, r, 4)


# ---- module level -----------------------------------------------------------------------------------
class Recorder:
    """Stands in for _lib.qconv2d_fused_bf16: records each call's arguments and result."""

    def __init__(self):
        self.real = _lib.qconv2d_fused_bf16
        self.calls = []

    def __call__(self, *args, **kw):
        y = self.real(*args, **kw)
        self.calls.append((args, kw, y))
        return y


def _module(mode="po2"):
    torch.manual_seed(41)
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
    res = torch.randn(2, 24, 9, 11).to(BF)
    return mod, bn, x, res


def _fold32(bn):
    """The test's own fp32 fold of a (bf16) BatchNorm: upcast, then s = rsqrt(var + eps) * weight and
    t = bias - mean * s in fp32."""
    with torch.no_grad():
        s = torch.rsqrt(bn.running_var.float() + bn.eps) * bn.weight.float()
        return s.cpu(), (bn.bias.float() - bn.running_mean.float() * s).cpu()


def test_switch_off_keeps_the_module_sequence(monkeypatch):
    assert qc.BF16_FUSED_EPILOGUE is False
    rec = Recorder()
    monkeypatch.setattr(_lib, "qconv2d_fused_bf16", rec)
    mod, bn, x, res = _module()
    with torch.no_grad():
        fused = mod.fused(x.to(DEV), bn, "relu", res.to(DEV))
        seq = _torch_epilogue(mod(x.to(DEV)), bn, "relu", res.to(DEV))
    assert torch.equal(_bits(fused), _bits(seq)) and rec.calls == []


@pytest.mark.parametrize("mode", ["po2", "po2+", None])
def test_switch_on_module_meets_the_fused_bar(monkeypatch, mode):
    monkeypatch.setattr(qc, "BF16_FUSED_EPILOGUE", True)
    rec = Recorder()
    monkeypatch.setattr(_lib, "qconv2d_fused_bf16", rec)
    mod, bn, x, res = _module(mode)
    with torch.no_grad():
        y = mod.fused(x.to(DEV), bn, "relu", res.to(DEV))
        y2 = mod.fused(x.to(DEV), bn, "relu", res.to(DEV))  # the cached fold
    assert len(rec.calls) == 2 and torch.equal(_bits(y), _bits(y2))
    s, t = _fold32(bn)
    ps, pb = rec.calls[0][1]["post_scale"], rec.calls[0][1]["post_shift"]
    assert ps.dtype == torch.float32 and torch.equal(ps.cpu(), s) and torch.equal(pb.cpu(), t)
    assert rec.calls[1][1]["post_scale"] is ps  # folded once
    w, b = mod.weight.detach().cpu(), mod.bias.detach().cpu()
    c, mag = reference(x, quantized(w, mode or "none"), b, 1, 1, 1, 1)
    assert_fused_bar(y.cpu(), c, mag, 20 * 9, s, t, res, "relu", "module", "module %s" % mode)


def test_switch_on_hooked_module_takes_the_unfused_path(monkeypatch):
    monkeypatch.setattr(qc, "BF16_FUSED_EPILOGUE", True)
    rec = Recorder()
    monkeypatch.setattr(_lib, "qconv2d_fused_bf16", rec)
    mod, bn, x, res = _module()
    seen = []
    mod.register_forward_hook(lambda m, inp, out: seen.append(out.detach().clone()))
    with torch.no_grad():
        fused = mod.fused(x.to(DEV), bn, "relu", res.to(DEV))
        conv = _lib.qconv2d_bf16(x.to(DEV), mod.weight, mod.bias, 1, 1, 1, 1, BITS, "po2")
        seq = _torch_epilogue(conv, bn, "relu", res.to(DEV))
    assert rec.calls == [] and len(seen) == 1
    assert torch.equal(_bits(seen[0]), _bits(conv))  # the hook got the conv's own output
    assert torch.equal(_bits(fused), _bits(seq))


def test_switch_on_requires_no_grad(monkeypatch):
    monkeypatch.setattr(qc, "BF16_FUSED_EPILOGUE", True)
    mod, bn, x, res = _module()
    with pytest.raises(_lib.Po2qError, match="no_grad"):
        mod.fused(x.to(DEV), bn, "relu", res.to(DEV))
    stem = nn.Conv2d(20, 24, 3, padding=1).bfloat16().to(DEV)
    with pytest.raises(_lib.Po2qError, match="no_grad"):
        qc.plain_conv_fused(stem, x.to(DEV), bn, "relu")


# ---- model level ------------------------------------------------------------------------------------
def _conv_bn_pairs(model):
    out = []
    for m in model.modules():
        ch = list(m.children())
        out += [c for c, nxt in zip(ch, ch[1:])
                if isinstance(c, nn.Conv2d) and isinstance(nxt, nn.modules.batchnorm._BatchNorm)]
    return out


@pytest.mark.parametrize("name", ["resnet20", "mobilenet"])
def test_model_layers_through_the_fused_entry(monkeypatch, name):
    """Every conv + BatchNorm of an eval bf16 forward runs as one fused call that meets the fused bar
    against fp64 computed from its own recorded inputs (no whole-model tolerance)."""
    monkeypatch.setattr(qc, "BF16_FUSED_EPILOGUE", True)
    rec = Recorder()
    monkeypatch.setattr(_lib, "qconv2d_fused_bf16", rec)
    torch.manual_seed(42)
    model = get_model(name, 10, quantizer_dict["po2"], BITS, (32, 32)).eval().bfloat16().to(DEV)
    x = torch.randn(2, 3, 32, 32).to(BF).to(DEV)
    with torch.no_grad():
        logits = model(x)
    assert logits.dtype == BF and tuple(logits.shape) == (2, 10) and bool(torch.isfinite(logits.float()).all())
    expected = _conv_bn_pairs(model)
    assert len(expected) == len([m for m in model.modules() if isinstance(m, nn.Conv2d)]) >= 19
    if name == "resnet20":
        assert model.conv1 in expected  # the stem
    called = {args[1].data_ptr() for args, _, _ in rec.calls}
    missing = [tuple(m.weight.shape) for m in expected if m.weight.data_ptr() not in called]
    assert not missing, "convs that did not take the fused entry: %s" % missing
    for args, kw, y in rec.calls:
        xi, w, b, stride, pad, dil, groups, bits, mode, fsr = args
        assert kw["post_scale"] is not None and kw["post_scale"].dtype == torch.float32
        q = quantized(w.detach().cpu(), mode, bits, fsr)
        c, mag = reference(xi.cpu(), q, b.detach().cpu() if b is not None else None, stride, pad, dil, groups)
        r = kw["residual"].cpu() if kw["residual"] is not None else None
        k = (w.shape[1]) * w.shape[2] * w.shape[3]
        assert_fused_bar(y.cpu(), c, mag, k, kw["post_scale"].cpu(), kw["post_shift"].cpu(), r, kw["act"],
                         "model-" + name, "%s %s" % (name, tuple(w.shape)))
