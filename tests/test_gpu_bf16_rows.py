"""GPU: the opt-in row-streaming bf16 conv kernel (conv_b16_rows<C, GW, EPI>, "kind=bf16_rows") behind the
bf16 entries, at the shapes of tests/_bf16_rows_cases.py (tests/test_bf16_rows_cpu.py pins that they
run it and which conditions they cover).

Reference, bar and exact operands are those of tests/test_gpu_bf16_conv_paths.py (plain entry) and
tests/test_gpu_bf16_fused.py (fused entry), reused as they stand: the kernel's arithmetic contract is
the tile kernel's, only the accumulation order may differ.  On exact_case operands every partial sum
is a multiple of 2^-7 below 4 k = 4 * 288, exact in fp32 in any order, so there the row kernel has to
give the fp64 reference's bits and the tile kernel's bits.

Every conv goes through the C ABI with y between sentinel bands (the run helpers of those two files).
The switch is process-wide: the fixture below turns it on for each test of this file and puts the
previous value back afterwards."""
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
from tests import test_gpu_bf16_conv_paths as paths
from tests import test_gpu_bf16_fused as fz
from tests._bf16_cases import BF, BITS, MODES, assert_bar, exact_case, quantized, random_case, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIAS = pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
TABLE_P = pytest.mark.parametrize("shape", rc.TABLE, ids=cases.case_id)
# both C, GW = 2 / 1 / 1 / 4, a ragged last group (82, 50, 130), a single masked group, one-row last bands
SUBSET = [rc.TABLE[7], rc.TABLE[8], rc.TABLE[3], rc.TABLE[10]]
SUBSET_P = pytest.mark.parametrize("shape", SUBSET, ids=cases.case_id)


@pytest.fixture(autouse=True)
def rows_on():
    with _lib.bf16_rows():
        yield


def _bits(t):
    return t.contiguous().view(torch.int16)


def dev(*ts):
    return tuple(t.to(DEV) if t is not None else None for t in ts)


def k_of(shape):
    return 9 * shape[1]


def is_rows(shape):
    return rc.describe(shape).startswith("kind=bf16_rows ")


@functools.lru_cache(maxsize=None)
def random_ref(shape, mode, bias):
    """(x, w, b, ref, mag) of a case, computed once and shared; nothing changes them afterwards."""
    x, w, b = random_case(shape, 1, 41, bias)
    ref, mag = reference(x, quantized(w, mode), b, *cases.conv_args(shape), 1)
    return x, w, b, ref, mag


# ---- every table shape: error bar and bit-exact -------------------------------------------------------
@BIAS
@pytest.mark.parametrize("mode", MODES)
@TABLE_P
def test_error_bar(shape, mode, bias):
    assert is_rows(shape)
    x, w, b, ref, mag = random_ref(shape, mode, bias)
    y = paths.run(*dev(x, w, b), shape, 1, mode)
    assert_bar(y, ref, mag, k_of(shape), "%s %s" % (shape, mode))


@BIAS
@pytest.mark.parametrize("mode", MODES)
@TABLE_P
def test_bit_exact_with_the_reference_and_the_tile_kernel(shape, mode, bias):
    assert is_rows(shape) and 4 * k_of(shape) * 128 < 2 ** 24  # the premise: 18 bits hold every partial sum
    x, w, b = exact_case(shape, 1, 42, bias, mode)
    q = quantized(w, mode)
    if mode != "none":
        assert bool((q.double() * 128 == (q.double() * 128).round()).all())  # the premise: multiples of 2^-7
    ref = F.conv2d(x.double(), q.double(), b.double() if b is not None else None, 1, 1).to(BF)
    xd, wd, bd = dev(x, w, b)
    y = paths.run(xd, wd, bd, shape, 1, mode)
    assert torch.equal(_bits(y), _bits(ref)), "%d of %d elements differ from the reference" % (int((y != ref).sum()), y.numel())
    with _lib.bf16_rows(False):
        assert not is_rows(shape)
        tile = paths.run(xd, wd, bd, shape, 1, mode)
    assert torch.equal(_bits(y), _bits(tile)), "%d elements differ from the tile kernel" % int((y != tile).sum())


# ---- fused epilogue ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", fz.TABLE, ids=lambda r: "%d%d%d-%s" % (r[0], r[1], r[2], r[3]))
@SUBSET_P
def test_fused_epilogue_error_bar(shape, row):
    assert is_rows(shape)
    fz.check_bar(shape, False, "po2", True, row, "rows")


@pytest.mark.parametrize("row", [(True, True, True, "relu"), (False, False, True, "none")], ids=["111-relu", "001-none"])
@SUBSET_P
def test_fused_epilogue_bit_exact(shape, row):
    """The exact operands of tests/test_gpu_bf16_fused.py::test_bit_exact (its docstring has the premise)."""
    has_s, has_t, has_r, act = row
    K = shape[4]
    x, w, b = exact_case(shape, 1, 43, True, "po2")
    c, mag = reference(x, quantized(w, "po2"), b, 1, 1, 1, 1)
    gen = torch.Generator().manual_seed(44)
    s = torch.tensor([0.5, 1.0, 2.0, -1.0, 0.25, -2.0])[torch.randint(0, 6, (K,), generator=gen)] if has_s else None
    t = torch.randint(-8, 9, (K,), generator=gen).float() / 8 if has_t else None
    r = (torch.randint(-32, 33, c.shape, generator=gen).float() / 8).to(BF) if has_r else None
    pre = c * (s.double().view(1, -1, 1, 1) if has_s else 1.0) + (t.double().view(1, -1, 1, 1) if has_t else 0.0) \
        + (r.double() if has_r else 0.0)
    assert bool((pre * 512 == (pre * 512).round()).all()) and float((2 * mag + 5).max()) * 512 < 2 ** 24
    ref = fz.act64(pre, act).to(BF)
    y = fz.run(*dev(x, w, b), shape, 1, "po2", *dev(s, t, r), fz.ACT_ID[act])
    assert torch.equal(_bits(y), _bits(ref)), "%d of %d elements differ" % (int((y != ref).sum()), y.numel())


@TABLE_P
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


def test_pack_batch_mixes_eligible_and_ineligible_layers():
    """(shape, groups, mode, bits, fsr) jobs through po2q_qconv2d_bf16_pack_batch, then
    po2q_qconv2d_packed_bf16: the bits of the one-call entry, workspaces and y between bands."""
    L = _lib.load()
    jobs = [(rc.TABLE[7], 1, 1, 4, 1), (rc.INELIGIBLE[0][0], 1, 2, 3, 1), (rc.TABLE[8], 1, 0, 4, 1),
            (rc.TABLE[3], 1, 2, 4, 2), (rc.INELIGIBLE[10][0], 16, 1, 5, 1), (rc.TABLE[9], 1, 1, 8, 1)]
    assert [is_rows(s) and g == 1 for s, g, _, _, _ in jobs] == [True, False, True, True, False, True]
    n = len(jobs)
    data, need, geo = [], [], []
    for i, (s, g, mode, nb, fsr) in enumerate(jobs):
        x, w, b = dev(*random_case(s, g, 45 + i, True))
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
        st = L.po2q_qconv2d_packed_bf16(x.data_ptr(), b.data_ptr(), ybuf.data_ptr() + BAND, *cases.geom14(s, g), nb, fsr,
                                        mode, None, None, None, 0, buf.data_ptr() + BAND, nbytes, _stream())
        assert st == 0, L.po2q_last_error()
        torch.cuda.synchronize()
        for t, inner in ((buf, nbytes), (ybuf, ybytes)):
            assert bool((t[:BAND] == FILL).all()) and bool((t[BAND + inner:] == FILL).all()), (s, "band overwritten")
        y = ybuf[BAND:BAND + ybytes].view(BF).view(s[0], s[4], P, Q).cpu()
        one_call = paths.run(x, w, b, s, g, MODE_NAME[mode], nb, fsr)
        assert torch.equal(_bits(y), _bits(one_call)), s


def test_packed_conv_refuses_a_workspace_sized_for_the_tile_plan():
    L = _lib.load()
    shape = rc.TABLE[7]
    geom = cases.geom14(shape)
    with _lib.bf16_rows(False):
        small = L.po2q_qconv2d_bf16_workspace_bytes(*geom, BITS, 1, 1)
    need = L.po2q_qconv2d_bf16_workspace_bytes(*geom, BITS, 1, 1)
    assert 0 < small < need  # C = 16: 6 KiB of row fragments against 5 KiB of tile fragments
    x, w, b = dev(*random_case(shape, 1, 46, True))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    y = torch.full((shape[0], shape[4], shape[2], shape[3]), -7.0, dtype=BF, device=DEV)
    st = L.po2q_qconv2d_packed_bf16(x.data_ptr(), b.data_ptr(), y.data_ptr(), *geom, BITS, 1, 1, None, None, None, 0,
                                    ws.data_ptr(), small, _stream())
    torch.cuda.synchronize()
    assert st == 3 and b"workspace" in L.po2q_last_error()  # PO2Q_ERR_WORKSPACE
    assert bool((y == -7.0).all()), "a refused call wrote y"


# ---- the conv's quantize-and-pack equals the native quantizer -------------------------------------------
@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("bits,fsr", paths.QUANT_WINDOWS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [rc.TABLE[7], rc.TABLE[9]], ids=cases.case_id)
def test_quantize_and_pack_equals_the_native_quantizer(shape, bits, fsr, mode):
    assert is_rows(shape)
    x, w, b = random_case(shape, 1, 47, True)
    q_cpu = _lib.restated_quantize(w, bits, mode, fsr)
    assert bool((q_cpu.float().abs() >= 2.0 ** -126).all())
    xd, wd, bd = dev(x, w, b)
    qd = _lib.quantize(wd, bits, mode, fsr)
    assert torch.equal(_bits(qd.cpu()), _bits(q_cpu))
    fused = paths.run(xd, wd, bd, shape, 1, mode, bits, fsr)
    two_step = paths.run(xd, qd.contiguous(), bd, shape, 1, "none")
    assert torch.equal(_bits(fused), _bits(two_step)), "%d elements differ" % int((fused != two_step).sum())
    ref, mag = reference(x, q_cpu, b, 1, 1, 1, 1)
    assert_bar(fused, ref, mag, k_of(shape), "%s bits %d fsr %d %s" % (shape, bits, fsr, mode))


# ---- alignment and layout -------------------------------------------------------------------------------
# W = 82: a row is 164 bytes, so 16-byte, 4-byte and (displaced) 2-byte stores all occur; W = 32 and 100 at both C
ALIGNMENT = [rc.TABLE[7], rc.TABLE[2], rc.TABLE[9]]


@pytest.mark.parametrize("which", ["x", "w", "bias", "y", "residual", "all"])
@pytest.mark.parametrize("shape", ALIGNMENT, ids=cases.case_id)
def test_two_byte_aligned_pointers(shape, which):
    assert is_rows(shape)
    x, w, b, c, mag, s, t, r = fz.random_ref(shape, False, "po2", True)
    x, w, b, s, t, r = dev(x, w, b, s, t, r)
    for v in (x, w, b, r):
        assert v.data_ptr() % 16 == 0
    want = fz.run(x, w, b, shape, 1, "po2", s, t, r, fz.ACT_ID["relu"])
    fz.assert_fused_bar(want, c, mag, k_of(shape), s.cpu(), t.cpu(), r.cpu(), "relu", "rows-aligned", "%s aligned" % (shape,))
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
NONFINITE = [rc.TABLE[10], rc.TABLE[8]]  # C = 16: 9 groups, 3 bands; C = 32: 4 groups, 2 bands, N = 3
INF, NAN = float("inf"), float("nan")


def places(shape):
    H, W = shape[2], shape[3]
    with _lib.bf16_rows():
        RB = rc.parse_rows(rc.describe(shape)).RB
    assert RB < H and 16 < W
    return {"interior": (H // 2, W // 2 + 1), "corner": (0, 0), "last": (H - 1, W - 1),
            "band_edge": (RB - 1, 3), "band_start": (RB, W - 2), "group_edge": (1, 15), "group_start": (2, 16)}


@pytest.mark.parametrize("value", [INF, -INF, NAN], ids=["pinf", "ninf", "nan"])
@pytest.mark.parametrize("where", ["interior", "corner", "last", "band_edge", "band_start", "group_edge", "group_start"])
@pytest.mark.parametrize("shape", NONFINITE, ids=cases.case_id)
def test_one_nonfinite_activation(shape, where, value):
    assert is_rows(shape)
    x, w, b = random_case(shape, 1, 48, True)
    assert bool((quantized(w, "po2") != 0).all())
    h, wc = places(shape)[where]
    x = x.clone()
    x[shape[0] - 1, 5, h, wc] = value
    paths.check_nonfinite(shape, False, x, w, b)


@pytest.mark.parametrize("shape", NONFINITE, ids=cases.case_id)
def test_nonfinite_activations_together(shape):
    x, w, b = random_case(shape, 1, 49, True)
    pl = places(shape)
    x = x.clone()
    x[0, 5, pl["interior"][0], pl["interior"][1]] = INF
    x[0, 5, pl["interior"][0], pl["interior"][1] + 1] = -INF
    x[0, 2, 0, 0] = -INF
    x[shape[0] - 1, 7, pl["last"][0], pl["last"][1]] = NAN
    x[shape[0] - 1, 3, pl["band_edge"][0], pl["band_edge"][1]] = INF
    x[1, 9, pl["group_edge"][0], pl["group_edge"][1]] = -INF
    paths.check_nonfinite(shape, False, x, w, b)


@pytest.mark.parametrize("shape", NONFINITE, ids=cases.case_id)
def test_nan_weight_stays_nan(shape):
    """An all-zero weight has max|w| = 0: Q(w) = 0 / 0 is NaN everywhere, and so is every output."""
    x, w, b = random_case(shape, 1, 50, True)
    w = torch.zeros_like(w)
    q = quantized(w, "po2")
    assert bool(torch.isnan(q.float()).all())
    ref = F.conv2d(x.double(), q.double(), b.double(), 1, 1)
    y = paths.run(*dev(x, w, b), shape, 1, "po2")
    assert bool(torch.isnan(ref).all()) and bool(torch.isnan(y.float()).all())


# ---- a model ----------------------------------------------------------------------------------------------
def test_resnet20_forward_under_the_switch():
    """Stages 1 and 2 (C = 16 @32, C = 32 @16) run the row kernel, stage 3 (C = 64) and the strided layers
    the tile kernel; every conv meets the layer bar of tests/test_gpu_bf16_conv.py::test_model_layers, which
    is that test's whole model-level criterion (it derives no tolerance on the logits: the layers' roundings
    compound).  The logits under both settings are printed; they must be finite, and the batched packs
    recorded under one setting are not consumed under the other (each setting reproduces its own bits)."""
    torch.manual_seed(18)
    model = get_model("resnet20", 10, quantizer_dict["po2"], BITS, (32, 32)).eval().bfloat16().to(DEV)
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    x = torch.randn(2, 3, 32, 32).to(BF).to(DEV)

    def forward(rec=None):
        hooks = [m.register_forward_hook(lambda mod, inp, out: rec.append((mod, inp[0].detach().cpu(), out.detach().cpu())))
                 for m in convs] if rec is not None else []
        try:
            with torch.no_grad():
                return model(x)
        finally:
            for h in hooks:
                h.remove()

    with _lib.bf16_rows(False):
        off = [forward(), forward()]  # the second consumes the packs the first recorded
    rec = []
    on = [forward(rec), forward(), forward()]
    with _lib.bf16_rows(False):
        off.append(forward())
    for ys in (on, off):
        assert all(torch.equal(_bits(y), _bits(ys[0])) for y in ys[1:])
        assert ys[0].dtype == BF and tuple(ys[0].shape) == (2, 10) and bool(torch.isfinite(ys[0].float()).all())
    print("max |logits(on) - logits(off)| = %.4g of max |logits| = %.4g"
          % ((on[0].float() - off[0].float()).abs().max().item(), off[0].float().abs().max().item()))
    assert {id(m) for m, _, _ in rec} == {id(m) for m in convs}
    kinds = {"rows": 0, "tile64": 0}
    for m, xi, yo in rec:
        N, C, H, W = xi.shape
        desc = _lib.describe_bf16(N, C, H, W, m.out_channels, *m.kernel_size, m.stride, m.padding, m.dilation, m.groups)
        eligible = (m.kernel_size == (3, 3) and m.stride == (1, 1) and m.in_channels == m.out_channels
                    and m.in_channels in (16, 32))
        assert desc.startswith("kind=bf16_rows ") == eligible, (tuple(m.weight.shape), desc)
        kinds["rows"] += eligible
        if m.in_channels == 64:
            assert desc.startswith("kind=bf16x1 "), desc
            kinds["tile64"] += 1
        w = m.weight.detach().cpu()
        mode = NATIVE_MODES.get(getattr(m, "quantize_fn", None))
        q = _lib.restated_quantize(w, m.bits, mode) if mode else w
        b = m.bias.detach().cpu() if m.bias is not None else None
        ref, mag = reference(xi, q, b, m.stride, m.padding, m.dilation, m.groups)
        assert_bar(yo, ref, mag, m.in_channels * m.kernel_size[0] * m.kernel_size[1], "resnet20 %s" % (tuple(w.shape),))
    assert kinds["rows"] == 11 and kinds["tile64"] >= 5, kinds  # 6 convs of stage 1, 5 of stage 2
