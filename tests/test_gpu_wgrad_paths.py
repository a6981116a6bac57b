"""GPU: every weight-gradient case of tests/_wgrad_cases.py through _lib.conv_wgrad -- all 32
register-streaming instances, long and ragged segments, the LDS-band kernel's tiles and bands, the
depthwise kernel's slices and tap templates (tests/test_wgrad_cases_cpu.py pins which case reaches
what) -- against aten.convolution_backward in fp64 on the CPU.

Two runs per case:
  * exact: x and dy are integers in [-4, 4].  Every product is an integer of magnitude <= 16 and
    every partial sum over (n, p, q), in any order, an integer below 16 N P Q < 2^24, so fp32 MFMA
    products, fp32 accumulation, the depthwise kernel's fp32 FMAs and every fixed-order reduction
    are exact: the result must EQUAL the fp64 reference.  One wrong, missing or doubled edge pixel
    changes an integer sum and cannot hide under a normwise bar.
  * randn: standard-normal operands under the project's bar, normwise CONV_TOL.
The three long-segment cases take their fp64 reference on the device as unfold(x) times dy (plain
torch ops); that helper is pinned against the CPU reference below."""
import pytest
import torch

from po2_quantization_amd import _lib
from tests import _wgrad_cases as cases
from tests._util import CONV_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def nerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def run(x, gy, shape, groups):
    stride, pad, dil = cases.conv_args(shape)
    return _lib.conv_wgrad(x, gy, cases.wshape(shape, groups), stride, pad, dil, groups)


def reference(x, gy, shape, groups):
    """x, gy on the device.  fp64: on the CPU, or on the device for the long-segment cases."""
    if shape in cases.LONG:
        return cases.reference_unfold(x, gy, shape)
    return cases.reference_cpu(x, gy, shape, groups)


IDS = [cases.case_id(s) + ("-dw" if g > 1 else "") for s, g in cases.RUN]


@pytest.mark.parametrize("shape,groups", cases.RUN, ids=IDS)
def test_wgrad_exact_on_small_integers(shape, groups):
    assert cases.exact_sums_fit(shape)
    x, gy = (t.to(DEV) for t in cases.operands(shape, sum(shape) + groups, exact=True))
    ref = reference(x, gy, shape, groups)
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) < 2 ** 24
    gw = run(x, gy, shape, groups)
    print(cases.case_id(shape), "max |gw - ref| = %g" % float((gw.cpu().double() - ref).abs().max()))
    assert torch.equal(gw.cpu().double(), ref)


@pytest.mark.parametrize("shape,groups", cases.RUN, ids=IDS)
def test_wgrad_randn_vs_fp64(shape, groups):
    x, gy = (t.to(DEV) for t in cases.operands(shape, sum(shape) + 7 * groups, exact=False))
    ref = reference(x, gy, shape, groups)
    gw = run(x, gy, shape, groups)
    print(cases.case_id(shape), "normwise error %.3g" % nerr(gw, ref))
    assert torch.isfinite(gw).all()
    assert nerr(gw, ref) <= CONV_TOL, nerr(gw, ref)


@pytest.mark.parametrize("shape", [cases.STREAM_GRID[0], cases.STREAM_GRID[12], cases.BAND[0], cases.BAND[4]],
                         ids=cases.case_id)
def test_device_reference_is_the_cpu_reference(shape):
    """reference_unfold (the long cases' reference) against aten.convolution_backward on the CPU: equal on
    integer operands, to fp64 rounding on normal ones."""
    x, gy = cases.operands(shape, 11, exact=True)
    assert torch.equal(cases.reference_unfold(x.to(DEV), gy.to(DEV), shape), cases.reference_cpu(x, gy, shape))
    x, gy = cases.operands(shape, 12, exact=False)
    assert nerr(cases.reference_unfold(x.to(DEV), gy.to(DEV), shape), cases.reference_cpu(x, gy, shape)) <= 1e-12


@pytest.mark.parametrize("shape,groups", [(cases.STREAM_EDGES[3], 1), (cases.BAND[0], 1), (cases.DEPTHWISE[0], 8)],
                         ids=["stream", "band", "depthwise"])
def test_wgrad_is_deterministic(shape, groups):
    x, gy = (t.to(DEV) for t in cases.operands(shape, 5, exact=False))
    assert torch.equal(run(x, gy, shape, groups), run(x, gy, shape, groups))  # fixed summation order, no atomics


def offset_view(t, floats):
    """A contiguous copy of t that starts `floats` fp32 elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    lead = (-buf.data_ptr() % 16) // 4 + floats  # elements to the next 16-byte boundary, then the offset
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (floats % 4)
    return v


@pytest.mark.parametrize("shape", cases.ALIGNMENT, ids=cases.case_id)
def test_wgrad_vec_loads_from_dword_aligned_tensors(shape):
    """vec = 1 is decided from W and Q alone and conv_wgrad keeps a contiguous view's storage offset, so
    the kernel's 16-byte buffer loads may start at any 4-byte-aligned address.  That is within what the
    hardware takes: the buffer addressing rules of AMD's GCN / CDNA ISA guides ask dword alignment of a
    dword-or-wider buffer access ("the two LSBs of the byte address are ignored"), not the access
    size's, for the descriptor base and the offset alike.  Bit for bit the aligned run."""
    assert cases.parse(cases.describe(shape))[1]["vec"] == 1
    x, gy = (t.to(DEV) for t in cases.operands(shape, 21, exact=False))
    assert x.data_ptr() % 16 == 0 and gy.data_ptr() % 16 == 0
    want = run(x, gy, shape, 1)
    assert nerr(want, cases.reference_cpu(x, gy, shape)) <= CONV_TOL
    for ox, og in ((1, 0), (0, 2), (3, 1), (2, 3)):
        got = run(offset_view(x, ox), offset_view(gy, og), shape, 1)
        assert torch.equal(got, want), (ox, og)
