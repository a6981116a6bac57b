"""GPU: the opt-in C = K = 64 row-streaming bf16 conv kernel (conv_b16_rowsk<GW, EPI>, "kind=bf16_rowsk")
behind the bf16 entries, at the shapes of tests/_bf16_rowsk_cases.py (tests/test_bf16_rowsk_cpu.py pins
that they run it and which conditions they cover).

Reference, bar and exact operands are those of tests/test_gpu_bf16_conv_paths.py (plain entry) and
tests/test_gpu_bf16_fused.py (fused entry), reused as they stand with k = 9 * 64 = 576: the kernel's
arithmetic contract is the tile kernel's, only the accumulation order may differ.  On exact_case operands
every partial sum is a multiple of 2^-7 below 4 k = 2304 (19 bits), exact in fp32 in any order, so there
the kernel has to give the fp64 reference's bits and the tile kernel's bits: a wrong wave-to-channel map,
tap, halo column or band edge shows there.

Every conv goes through the C ABI with y between sentinel bands (the run helpers of those two files).
The switch is process-wide: the fixture below turns it on for each test of this file (the first row
kernel's switch stays as it is, off, unless a test says otherwise) and puts the previous value back."""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from po2_quantization_amd import _lib
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.utils.quantizers import NATIVE_MODES, quantizer_dict
from tests import _bf16_cases as cases
from tests import _bf16_rows_cases as rc
from tests import _bf16_rowsk_cases as kc
from tests import _nonfinite
from tests import test_gpu_bf16_conv_paths as paths
from tests import test_gpu_bf16_fused as fz
from tests._bf16_cases import BF, BITS, MODES, assert_bar, exact_case, quantized, random_case, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K576 = 9 * kc.C
BIAS = pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
TABLE_P = pytest.mark.parametrize("shape", kc.TABLE, ids=cases.case_id)
# GW = 2 with a ragged group and band, GW = 4 with an idle slot, W = 56 with N = 3, GW = 1 half-filled
SUBSET = [kc.TABLE[4], kc.TABLE[5], kc.TABLE[6], kc.TABLE[2]]
SUBSET_P = pytest.mark.parametrize("shape", SUBSET, ids=cases.case_id)


@pytest.fixture(autouse=True)
def rowsk_on():
    with _lib.bf16_rowsk():
        yield


def _bits(t):
    return t.contiguous().view(torch.int16)


def dev(*ts):
    return tuple(t.to(DEV) if t is not None else None for t in ts)


@functools.lru_cache(maxsize=None)
def _conv_ref(shape, mode):
    """(ref, mag) without bias in fp64, once per (shape, mode): the two bias variants share it."""
    x, w, _ = random_case(shape, 1, 61, False)
    return reference(x, quantized(w, mode), None, *cases.conv_args(shape), 1)


def random_ref(shape, mode, bias):
    """(x, w, b, ref, mag) of a case; x and w do not depend on `bias` (random_case draws b last)."""
    x, w, b = random_case(shape, 1, 61, bias)
    ref, mag = _conv_ref(shape, mode)
    if b is not None:
        ref, mag = ref + b.double().view(1, -1, 1, 1), mag + b.double().abs().view(1, -1, 1, 1)
    return x, w, b, ref, mag


# ---- every table shape: error bar and bit-exact -------------------------------------------------------
@BIAS
@pytest.mark.parametrize("mode", MODES)
@TABLE_P
def test_error_bar(shape, mode, bias):
    assert kc.is_rowsk(shape)
    x, w, b, ref, mag = random_ref(shape, mode, bias)
    y = paths.run(*dev(x, w, b), shape, 1, mode)
    assert_bar(y, ref, mag, K576, "%s %s" % (shape, mode))


@functools.lru_cache(maxsize=None)
def _exact_ref(shape, mode):
    x, w, _ = exact_case(shape, 1, 62, False, mode)
    q = quantized(w, mode)
    if mode != "none":
        assert bool((q.double() * 128 == (q.double() * 128).round()).all())  # the premise: multiples of 2^-7
    return F.conv2d(x.double(), q.double(), None, 1, 1)


@BIAS
@pytest.mark.parametrize("mode", MODES)
@TABLE_P
def test_bit_exact_with_the_reference_and_the_tile_kernel(shape, mode, bias):
    assert kc.is_rowsk(shape) and 4 * K576 * 128 < 2 ** 24  # the premise: 19 bits hold every partial sum
    x, w, b = exact_case(shape, 1, 62, bias, mode)  # x, w as in _exact_ref: b is drawn last
    ref = _exact_ref(shape, mode)
    ref = (ref + b.double().view(1, -1, 1, 1) if bias else ref).to(BF)  # sums of multiples of 2^-7: exact in fp64
    xd, wd, bd = dev(x, w, b)
    y = paths.run(xd, wd, bd, shape, 1, mode)
    assert torch.equal(_bits(y), _bits(ref)), "%d of %d elements differ from the reference" % (int((y != ref).sum()), y.numel())
    with _lib.bf16_rowsk(False):
        assert cases.describe(shape).startswith("kind=bf16x1 ")
        tile = paths.run(xd, wd, bd, shape, 1, mode)
    assert torch.equal(_bits(y), _bits(tile)), "%d elements differ from the tile kernel" % int((y != tile).sum())


# ---- fused epilogue ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", fz.TABLE, ids=lambda r: "%d%d%d-%s" % (r[0], r[1], r[2], r[3]))
@SUBSET_P
def test_fused_epilogue_error_bar(shape, row):
    """BN + ReLU, BN + residual + ReLU, residual alone, ReLU6, SiLU and ReLU alone (fz.TABLE) under the
    fused bar of tests/test_gpu_bf16_fused.py."""
    assert kc.is_rowsk(shape)
    fz.check_bar(shape, False, "po2", True, row, "rowsk")


EXACT_ROWS = [(True, True, False, "none"), (True, True, False, "relu"), (True, True, True, "relu"),
              (True, False, False, "relu6"), (False, False, True, "none")]


@pytest.mark.parametrize("row", EXACT_ROWS, ids=lambda r: "%d%d%d-%s" % (r[0], r[1], r[2], r[3]))
@SUBSET_P
def test_fused_epilogue_bit_exact(shape, row):
    """The exact operands of tests/test_gpu_bf16_fused.py::test_bit_exact (its docstring has the premise):
    BN alone, BN + ReLU, BN + residual + ReLU, ReLU6 and the residual alone.  (SiLU has no exact operands:
    it is held to the bar above.)"""
    has_s, has_t, has_r, act = row
    K = shape[4]
    x, w, b = exact_case(shape, 1, 63, True, "po2")
    c, mag = reference(x, quantized(w, "po2"), b, 1, 1, 1, 1)
    gen = torch.Generator().manual_seed(64)
    s = torch.tensor([0.5, 1.0, 2.0, -1.0, 0.25, -2.0])[torch.randint(0, 6, (K,), generator=gen)] if has_s else None
    t = torch.randint(-8, 9, (K,), generator=gen).float() / 8 if has_t else None
    r = (torch.randint(-32, 33, c.shape, generator=gen).float() / 8).to(BF) if has_r else None
    pre = c * (s.double().view(1, -1, 1, 1) if has_s else 1.0) + (t.double().view(1, -1, 1, 1) if has_t else 0.0) \
        + (r.double() if has_r else 0.0)
    assert bool((pre * 512 == (pre * 512).round()).all()) and float((2 * mag + 5).max()) * 512 < 2 ** 24
    ref = fz.act64(pre, act).to(BF)
    y = fz.run(*dev(x, w, b), shape, 1, "po2", *dev(s, t, r), fz.ACT_ID[act])
    assert torch.equal(_bits(y), _bits(ref)), "%d of %d elements differ" % (int((y != ref).sum()), y.numel())


@pytest.mark.parametrize("shape", kc.TABLE[:8], ids=cases.case_id)
def test_identity_epilogue_equals_the_plain_entry(shape):
    x, w, b, _, _ = random_ref(shape, "po2", True)
    xd, wd, bd = dev(x, w, b)
    plain = fz.run(xd, wd, bd, shape, 1, "po2", plain=True)
    ident = fz.run(xd, wd, bd, shape, 1, "po2")
    assert torch.equal(_bits(ident), _bits(plain))


# ---- batched packs ------------------------------------------------------------------------------------
BAND, FILL = 512, 0xA5
MODE_NAME = ("none", "po2", "po2+")


def _stream():
    return _lib._stream(torch.device(DEV))


def test_pack_batch_mixes_rowsk_rows_tile_and_depthwise_jobs():
    """(shape, groups, mode, bits, fsr) jobs through po2q_qconv2d_bf16_pack_batch with both switches on, then
    po2q_qconv2d_packed_bf16: the bits of the one-call entry, workspaces and y between bands."""
    L = _lib.load()
    jobs = [(kc.TABLE[4], 1, 1, 4, 1), (rc.TABLE[7], 1, 2, 3, 1), (kc.INELIGIBLE[0][0], 1, 1, 4, 1),
            (kc.TABLE[6], 1, 0, 4, 1), (kc.INELIGIBLE[11][0], 64, 1, 5, 1), (kc.TABLE[5], 1, 2, 4, 2),
            (rc.TABLE[8], 1, 1, 8, 1)]
    with _lib.bf16_rows():
        kinds = [cases.describe(s, g).split()[0] for s, g, _, _, _ in jobs]
        assert kinds == ["kind=bf16_rowsk", "kind=bf16_rows", "kind=bf16x1", "kind=bf16_rowsk", "kind=dw_bf16",
                         "kind=bf16_rowsk", "kind=bf16_rows"]
        n = len(jobs)
        data, need, geo = [], [], []
        for i, (s, g, mode, nb, fsr) in enumerate(jobs):
            x, w, b = dev(*random_case(s, g, 65 + i, True))
            data.append((x, w, b))
            need.append(L.po2q_qconv2d_bf16_workspace_bytes(*cases.geom14(s, g), nb, fsr, mode))
            assert need[-1] > 0
            geo += list(cases.geom14(s, g))
        bufs = [torch.full((nbytes + 2 * BAND,), FILL, dtype=torch.uint8, device=DEV) for nbytes in need]
        st = L.po2q_qconv2d_bf16_pack_batch(
            n, (ctypes.c_void_p * n)(*[w.data_ptr() for _, w, _ in data]), (ctypes.c_int64 * len(geo))(*geo),
            (ctypes.c_int * n)(*[j[3] for j in jobs]), (ctypes.c_int * n)(*[j[4] for j in jobs]),
            (ctypes.c_int * n)(*[j[2] for j in jobs]), (ctypes.c_void_p * n)(*[b.data_ptr() + BAND for b in bufs]),
            (ctypes.c_size_t * n)(*need), _stream())
        assert st == 0, L.po2q_last_error()
        for (s, g, mode, nb, fsr), (x, w, b), buf, nbytes in zip(jobs, data, bufs, need):
            P, Q = cases.out_size(s)
            ybytes = s[0] * s[4] * P * Q * 2
            ybuf = torch.full((ybytes + 2 * BAND,), FILL, dtype=torch.uint8, device=DEV)
            st = L.po2q_qconv2d_packed_bf16(x.data_ptr(), b.data_ptr(), ybuf.data_ptr() + BAND, *cases.geom14(s, g), nb,
                                            fsr, mode, None, None, None, 0, buf.data_ptr() + BAND, nbytes, _stream())
            assert st == 0, L.po2q_last_error()
            torch.cuda.synchronize()
            for t, inner in ((buf, nbytes), (ybuf, ybytes)):
                assert bool((t[:BAND] == FILL).all()) and bool((t[BAND + inner:] == FILL).all()), (s, "band overwritten")
            y = ybuf[BAND:BAND + ybytes].view(BF).view(s[0], s[4], P, Q).cpu()
            one_call = paths.run(x, w, b, s, g, MODE_NAME[mode], nb, fsr)
            assert torch.equal(_bits(y), _bits(one_call)), s


def test_a_workspace_one_byte_short_is_refused_with_y_untouched():
    L = _lib.load()
    shape = kc.TABLE[4]
    geom = cases.geom14(shape)
    need = L.po2q_qconv2d_bf16_workspace_bytes(*geom, BITS, 1, 1)
    with _lib.bf16_rowsk(False):
        assert need < L.po2q_qconv2d_bf16_workspace_bytes(*geom, BITS, 1, 1)  # the tile plan pads its k-steps
    assert need == 1024 + 4 * 18 * 1024
    x, w, b = dev(*random_case(shape, 1, 66, True))
    assert fz.run(x, w, b, shape, 1, "po2", act=fz.ACT_ID["relu"], refused=True, ws_cut=1) is None
    assert fz.run(x, w, b, shape, 1, "po2", plain=True, refused=True, ws_cut=1) is None
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    y = torch.full((shape[0], shape[4], shape[2], shape[3]), -7.0, dtype=BF, device=DEV)
    st = L.po2q_qconv2d_packed_bf16(x.data_ptr(), b.data_ptr(), y.data_ptr(), *geom, BITS, 1, 1, None, None, None, 0,
                                    ws.data_ptr(), need - 1, _stream())
    torch.cuda.synchronize()
    assert st == 3 and b"workspace" in L.po2q_last_error()  # PO2Q_ERR_WORKSPACE
    assert bool((y == -7.0).all()), "a refused call wrote y"
    wptr, wsp, nb = (ctypes.c_void_p * 1)(w.data_ptr()), (ctypes.c_void_p * 1)(ws.data_ptr()), (ctypes.c_size_t * 1)(need - 1)
    one = (ctypes.c_int * 1)
    st = L.po2q_qconv2d_bf16_pack_batch(1, wptr, (ctypes.c_int64 * 14)(*geom), one(BITS), one(1), one(1), wsp, nb, _stream())
    torch.cuda.synchronize()
    assert st == 3 and bool((ws == 0).all()), "a refused pack batch wrote its workspace"


# ---- the conv's quantize-and-pack equals the native quantizer -------------------------------------------
@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("bits,fsr", paths.QUANT_WINDOWS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [kc.TABLE[4], kc.TABLE[6]], ids=cases.case_id)
def test_quantize_and_pack_equals_the_native_quantizer(shape, bits, fsr, mode):
    assert kc.is_rowsk(shape)
    x, w, b = random_case(shape, 1, 67, True)
    q_cpu = _lib.restated_quantize(w, bits, mode, fsr)
    assert bool((q_cpu.float().abs() >= 2.0 ** -126).all())
    xd, wd, bd = dev(x, w, b)
    qd = _lib.quantize(wd, bits, mode, fsr)
    assert torch.equal(_bits(qd.cpu()), _bits(q_cpu))
    fused = paths.run(xd, wd, bd, shape, 1, mode, bits, fsr)
    two_step = paths.run(xd, qd.contiguous(), bd, shape, 1, "none")
    assert torch.equal(_bits(fused), _bits(two_step)), "%d elements differ" % int((fused != two_step).sum())
    ref, mag = reference(x, q_cpu, b, 1, 1, 1, 1)
    assert_bar(fused, ref, mag, K576, "%s bits %d fsr %d %s" % (shape, bits, fsr, mode))


# ---- alignment and layout -------------------------------------------------------------------------------
# W = 18: a row is 36 bytes, so 16-byte, 4-byte and (displaced) 2-byte pieces all occur; W = 34 (68 bytes, the
# GW = 4 instance with an idle slot) and W = 56 (112 bytes: every aligned piece 16 bytes)
ALIGNMENT = [kc.TABLE[4], kc.TABLE[5], kc.TABLE[6]]


@pytest.mark.parametrize("which", ["x", "w", "bias", "y", "residual", "all"])
@pytest.mark.parametrize("shape", ALIGNMENT, ids=cases.case_id)
def test_two_byte_aligned_pointers(shape, which):
    assert kc.is_rowsk(shape)
    x, w, b, c, mag, s, t, r = fz.random_ref(shape, False, "po2", True)
    x, w, b, s, t, r = dev(x, w, b, s, t, r)
    for v in (x, w, b, r):
        assert v.data_ptr() % 16 == 0
    want = fz.run(x, w, b, shape, 1, "po2", s, t, r, fz.ACT_ID["relu"])
    fz.assert_fused_bar(want, c, mag, K576, s.cpu(), t.cpu(), r.cpu(), "relu", "rowsk-aligned", "%s aligned" % (shape,))
    xs, ws, bs, rs = (paths.displaced(v) if which in (name, "all") else v
                      for v, name in ((x, "x"), (w, "w"), (b, "bias"), (r, "residual")))
    got = fz.run(xs, ws, bs, shape, 1, "po2", s, t, rs, fz.ACT_ID["relu"], y_shift=1 if which in ("y", "all") else 0)
    assert torch.equal(_bits(got), _bits(want)), "%d of %d elements differ" % (int((got != want).sum()), got.numel())
    if which in ("x", "y", "all"):  # the plain instance's staging and stores as well
        wantp = paths.run(x, w, b, shape, 1, "po2")
        gotp = paths.run(xs, ws, bs, shape, 1, "po2", y_shift=1 if which in ("y", "all") else 0)
        assert torch.equal(_bits(gotp), _bits(wantp))


@pytest.mark.parametrize("shape", ALIGNMENT, ids=cases.case_id)
def test_channels_last_and_strided_inputs(shape):
    x, w, b, ref, mag = random_ref(shape, "po2", True)
    x, w, b = dev(x, w, b)
    want = paths.run(x, w, b, shape, 1, "po2")
    y = _lib.qconv2d_bf16(x, w, b, 1, 1, 1, 1, BITS, "po2").cpu()  # the wrapper and the op run what the C ABI runs
    assert torch.equal(_bits(y), _bits(want))
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert torch.equal(_bits(_lib.qconv2d_bf16(cl, w, b, 1, 1, 1, 1, BITS, "po2").cpu()), _bits(want))
    wide = torch.zeros(shape[0], shape[1] + 3, shape[2] + 2, shape[3] + 5, dtype=BF, device=DEV)
    sl = wide[:, 2:2 + shape[1], 1:1 + shape[2], 3:3 + shape[3]]
    sl.copy_(x)
    assert not sl.is_contiguous()
    wwide = torch.zeros(shape[4], shape[1] * 2, 3, 3, dtype=BF, device=DEV)
    wsl = wwide[:, ::2]
    wsl.copy_(w)
    assert torch.equal(_bits(_lib.qconv2d_bf16(sl, wsl, b, 1, 1, 1, 1, BITS, "po2").cpu()), _bits(want))


# ---- non-finite values ----------------------------------------------------------------------------------
NONFINITE = [kc.TABLE[4], kc.TABLE[6]]  # 2 groups, 3 bands, N = 2; 4 groups, 2 bands, N = 3
INF, NAN = float("inf"), float("nan")


def places(shape):
    H, W = shape[2], shape[3]
    RB = kc.parse_rowsk(kc.describe(shape)).RB
    assert RB < H and 16 < W
    return {"interior": (H // 2, W // 2 + 1), "corner": (0, 0), "last": (H - 1, W - 1),
            "band_edge": (RB - 1, 3), "band_start": (RB, W - 2), "group_edge": (1, 15), "group_start": (2, 16)}


@pytest.mark.parametrize("value", [INF, -INF, NAN], ids=["pinf", "ninf", "nan"])
@pytest.mark.parametrize("where", ["interior", "corner", "last", "band_edge", "band_start", "group_edge", "group_start"])
@pytest.mark.parametrize("shape", NONFINITE, ids=cases.case_id)
def test_one_nonfinite_activation(shape, where, value):
    assert kc.is_rowsk(shape)
    x, w, b = random_case(shape, 1, 68, True)
    assert bool((quantized(w, "po2") != 0).all())
    h, wc = places(shape)[where]
    x = x.clone()
    x[shape[0] - 1, 37, h, wc] = value
    paths.check_nonfinite(shape, False, x, w, b)


@pytest.mark.parametrize("shape", NONFINITE, ids=cases.case_id)
def test_nonfinite_activations_together(shape):
    x, w, b = random_case(shape, 1, 69, True)
    pl = places(shape)
    x = x.clone()
    x[0, 5, pl["interior"][0], pl["interior"][1]] = INF
    x[0, 5, pl["interior"][0], pl["interior"][1] + 1] = -INF
    x[0, 2, 0, 0] = -INF
    x[shape[0] - 1, 63, pl["last"][0], pl["last"][1]] = NAN
    x[shape[0] - 1, 33, pl["band_edge"][0], pl["band_edge"][1]] = INF
    x[1, 48, pl["group_edge"][0], pl["group_edge"][1]] = -INF
    paths.check_nonfinite(shape, False, x, w, b)


@pytest.mark.parametrize("shape", NONFINITE, ids=cases.case_id)
def test_nan_weight_stays_nan(shape):
    """An all-zero weight has max|w| = 0: Q(w) = 0 / 0 is NaN everywhere, and so is every output, as the tile
    kernel gives it."""
    x, w, b = random_case(shape, 1, 70, True)
    w = torch.zeros_like(w)
    q = quantized(w, "po2")
    assert bool(torch.isnan(q.float()).all())
    ref = F.conv2d(x.double(), q.double(), b.double(), 1, 1)
    xd, wd, bd = dev(x, w, b)
    y = paths.run(xd, wd, bd, shape, 1, "po2")
    assert bool(torch.isnan(ref).all()) and bool(torch.isnan(y.float()).all())
    with _lib.bf16_rowsk(False):
        tile = paths.run(xd, wd, bd, shape, 1, "po2")
    assert _nonfinite.same_nonfinite(y.float(), tile.float()) and _nonfinite.same_nonfinite(y.double(), ref)


# ---- a model ----------------------------------------------------------------------------------------------
def test_resnet20_forward_with_both_switches_on():
    """Stages 1 and 2 (C = 16 @32, C = 32 @16) run the first row kernel, stage 3's 3x3 stride-1 64 -> 64 convs
    (@8) the new one, the strided layers the tile kernel; every conv meets the layer bar of
    tests/test_gpu_bf16_conv.py::test_model_layers, which is that test's whole model-level criterion (it
    derives no tolerance on the logits: the layers' roundings compound).  The logits difference against
    both-off is printed; the batched packs recorded under one pair of settings are not consumed under
    another (each reproduces its own bits, whatever ran in between)."""
    torch.manual_seed(19)
    model = get_model("resnet20", 10, quantizer_dict["po2"], BITS, (32, 32)).eval().bfloat16().to(DEV)
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    x = torch.randn(2, 3, 32, 32).to(BF).to(DEV)

    def forward(first, new, rec=None):
        hooks = [m.register_forward_hook(lambda mod, inp, out: rec.append((mod, inp[0].detach().cpu(), out.detach().cpu())))
                 for m in convs] if rec is not None else []
        try:
            with torch.no_grad(), _lib.bf16_rows(first), _lib.bf16_rowsk(new):
                return model(x)
        finally:
            for h in hooks:
                h.remove()

    settings = [(False, False), (True, True), (False, True), (True, False)]
    outs = {st: [forward(*st), forward(*st)] for st in settings}  # the second consumes the packs the first recorded
    rec = []
    outs[(True, True)].append(forward(True, True, rec))
    for st in reversed(settings):
        outs[st].append(forward(*st))
    for st, ys in outs.items():
        assert all(torch.equal(_bits(y), _bits(ys[0])) for y in ys[1:]), st
        assert ys[0].dtype == BF and tuple(ys[0].shape) == (2, 10) and bool(torch.isfinite(ys[0].float()).all())
    off, on = outs[(False, False)][0], outs[(True, True)][0]
    print("max |logits(both on) - logits(both off)| = %.4g of max |logits| = %.4g"
          % ((on.float() - off.float()).abs().max().item(), off.float().abs().max().item()))
    assert {id(m) for m, _, _ in rec} == {id(m) for m in convs}
    kinds = {"rows": 0, "rowsk": 0}
    with _lib.bf16_rows():
        for m, xi, yo in rec:
            N, C, H, W = xi.shape
            desc = _lib.describe_bf16(N, C, H, W, m.out_channels, *m.kernel_size, m.stride, m.padding, m.dilation, m.groups)
            plain = m.kernel_size == (3, 3) and m.stride == (1, 1) and m.in_channels == m.out_channels
            assert desc.startswith("kind=bf16_rows ") == (plain and m.in_channels in (16, 32)), (tuple(m.weight.shape), desc)
            assert desc.startswith("kind=bf16_rowsk ") == (plain and m.in_channels == 64), (tuple(m.weight.shape), desc)
            kinds["rows"] += desc.startswith("kind=bf16_rows ")
            kinds["rowsk"] += desc.startswith("kind=bf16_rowsk ")
            w = m.weight.detach().cpu()
            mode = NATIVE_MODES.get(getattr(m, "quantize_fn", None))
            q = _lib.restated_quantize(w, m.bits, mode) if mode else w
            b = m.bias.detach().cpu() if m.bias is not None else None
            ref, mag = reference(xi, q, b, m.stride, m.padding, m.dilation, m.groups)
            assert_bar(yo, ref, mag, m.in_channels * m.kernel_size[0] * m.kernel_size[1], "resnet20 %s" % (tuple(w.shape),))
    assert kinds["rows"] == 11 and kinds["rowsk"] >= 5, kinds  # 6 convs of stage 1, 5 of stage 2, 5 of stage 3
