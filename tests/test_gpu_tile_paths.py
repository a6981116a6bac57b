"""GPU: every instance of the general-geometry fp32-forward kernels -- conv_bf16x3 (kind bf16x3), conv_x3p (kind
bf16x3_dma), conv_mfma_f32 and the legacy conv_depthwise -- through the rows of tests/_tile_cases.py, against the
oracle (fp64 direct conv of the bit-exact Q(w)) at the project's parity bar CONV_TOL (normwise).
tests/test_tile_cases_cpu.py proves on the host that the rows reach every instance the planners can produce and
that each row's forced tile is the plan that runs; here each row's plan is looked up the same way and run by its
candidate index through the C ABI (which plans on every call, so it obeys the tile knobs)."""
import numpy as np
import pytest
import torch

from tests import _tile_cases as T
from tests._nonfinite import nonfinite_input, same_nonfinite
from tests._util import CONV_TOL, normwise_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("po2", "po2+")
CHUNK = 8


def _dev(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


def _check_row(shape, index, env, seed, precision="auto", what=None):
    """Candidate `index` under `env` in po2 and po2+, with and without bias, against the oracle."""
    x, w, b = T.inputs(shape, seed)
    xd, wd, bd = _dev(x, w, b)
    for mode in MODES:
        ref = T.reference(x, w, shape, mode)
        for bias, r in ((None, ref), (bd, T.with_bias(ref, b))):
            y = T.run_plan(index(mode), xd, wd, bias, shape, env, mode, precision=precision).cpu().numpy()
            assert y.shape == r.shape
            err = normwise_err(y, r)
            assert err <= CONV_TOL, (what or shape, mode, bias is not None, err)


TILE_ROWS = T.X3_ROWS + T.X3_EDGES + T.DMA_ROWS + T.DMA_EDGES
TILE_CHUNKS = [TILE_ROWS[i:i + CHUNK] for i in range(0, len(TILE_ROWS), CHUNK)]


@pytest.mark.parametrize("rows", TILE_CHUNKS, ids=["%s-%03d" % (T.row_kind(c[0]), i * CHUNK)
                                                    for i, c in enumerate(TILE_CHUNKS)])
def test_tile_kernel_rows_vs_oracle(rows):
    for n, row in enumerate(rows):
        def index(mode, row=row):
            f = T.find_plan(row, mode)
            assert f is not None, (T.row_id(row), mode)
            return f[0]
        _check_row(row[0], index, T.row_env(row), 1000 + n, what=(T.row_kind(row), T.row_id(row), row[2]))


@pytest.mark.parametrize("row", T.MFMA_ROWS, ids=["x".join(map(str, r[0])) for r in T.MFMA_ROWS])
def test_fp32_mfma_rows_vs_oracle(row):
    """conv_mfma_f32<MI, NJ>: all nine instances, grouped convs, ragged channel chunks, stride-2 plane padding,
    7x7 (the ImageNet stem and its stride-1 sibling) and 9x9 -- also in mode none, which the kernel serves too."""
    shape, prec, key = row
    for mode in MODES:
        p = T.parse(T.describe(shape, mode=mode, precision=prec))
        assert p.kind == "mfma_f32" and T.instance_key(p) == key, p
    _check_row(shape, lambda mode: 0, None, sum(shape), precision=prec)
    # mode none: the same plan, behind the direct / pointwise fp32 kernels where those apply
    found = [(i, T.parse(d)) for i, d in enumerate(T.plans(shape, mode="none", precision=prec))]
    found = [(i, p) for i, p in found if p.kind == "mfma_f32"]
    assert found and T.instance_key(found[0][1]) == key, found
    x, w, b = T.inputs(shape, 7 + sum(shape))
    xd, wd, bd = _dev(x, w, b)
    ref = T.with_bias(T.reference(x, w, shape, "none"), b)
    y = T.run_plan(found[0][0], xd, wd, bd, shape, None, "none", precision=prec).cpu().numpy()
    assert normwise_err(y, ref) <= CONV_TOL, normwise_err(y, ref)


@pytest.mark.parametrize("shape", T.DEPTHWISE_ROWS, ids=["x".join(map(str, s)) for s in T.DEPTHWISE_ROWS])
def test_legacy_depthwise_rows_vs_oracle(shape):
    assert T.describe(shape).startswith("kind=depthwise CC=1 NT=0 MI=1 NJ=1 vr=0 ")
    _check_row(shape, lambda mode: 0, None, sum(shape))


@pytest.mark.parametrize("row", T.MULTI_ITEM_ROWS, ids=[T.row_id(r) + "-" + "".join(map(str, r[2]))
                                                         for r in T.MULTI_ITEM_ROWS])
def test_more_than_one_work_item_per_block(row):
    """A batch large enough that every block of the persistent grid walks at least four tiles: the counted vmcnt
    waits (which depend on the stores issued per tile), the 3-slot weight ring, the two x register sets / raw
    slots and, with ov = 1, the overlapped split all carry state from one work item to the next only then.  The
    batch is two distinct images repeated, so the oracle runs on two images and every output image is compared
    with its reference -- which also catches a block that mixes up image indices."""
    kind = T.row_kind(row)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _, p2 = T.find_plan(row)
    threads = 256 if kind == "bf16x3" else 64 * p2.waves
    resident = min(2048 // threads, (160 * 1024) // p2.lds)
    per_image = p2.blocks // row[0][0]
    N = -(-4 * resident * cus // per_image)
    shape = (N,) + row[0][1:]
    found = T.find_plan(row, "po2+", shape=shape)
    assert found is not None, shape
    index, p = found
    assert p.blocks >= 4 * min(2048 // threads, (160 * 1024) // p.lds) * cus, (p, cus)
    base, w, b = T.inputs(row[0], 77)
    ref = torch.from_numpy(T.with_bias(T.reference(base, w, row[0], "po2+"), b)).to(DEV)
    xd = base.to(DEV)[torch.arange(N, device=DEV) % 2].contiguous()
    wd, bd = _dev(w, b)
    y = T.run_plan(index, xd, wd, bd, shape, T.row_env(row), "po2+")
    amax = ref.abs().max().item()
    for j in (0, 1):
        err = (y[j::2].double() - ref[j]).abs().amax(dim=(1, 2, 3)) / amax
        worst = int(err.argmax())
        assert err.max().item() <= CONV_TOL, (j, "image", 2 * worst + j, err.max().item())


ACTS = ("none", "relu", "relu6", "silu")


def _check_fused(shape, index, env, precision, seed):
    x, w, b = T.inputs(shape, seed)
    P, Q = T.out_size(shape)
    g = torch.Generator().manual_seed(seed + 1)
    K = shape[4]
    ps, pb = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    res = torch.randn(shape[0], K, P, Q, generator=g)
    xd, wd, bd, psd, pbd, rd = _dev(x, w, b, ps, pb, res)
    conv = T.with_bias(T.reference(x, w, shape, "po2"), b)
    for act in ACTS:
        for r_t, r_d in ((None, None), (res, rd)):
            ref = T.epilogue(conv, ps, pb, r_t, act)
            y = T.run_fused(index, xd, wd, bd, shape, env, "po2", precision=precision, post_scale=psd, post_shift=pbd,
                            residual=r_d, act=act).cpu().numpy()
            err = normwise_err(y, ref)
            assert err <= CONV_TOL, (shape, act, r_t is not None, err)
    # activation alone (no affine, no residual), and the affine halves on their own
    for kw, ref in (({"act": "relu"}, T.epilogue(conv, act="relu")),
                    ({"post_scale": psd}, T.epilogue(conv, ps=ps)),
                    ({"post_shift": pbd, "residual": rd}, T.epilogue(conv, pb=pb, res=res))):
        y = T.run_fused(index, xd, wd, bd, shape, env, "po2", precision=precision, **kw).cpu().numpy()
        assert normwise_err(y, ref) <= CONV_TOL, (shape, sorted(kw))


@pytest.mark.parametrize("row", T.FUSED_TILE_ROWS, ids=[T.row_id(r) for r in T.FUSED_TILE_ROWS])
def test_fused_entry_on_the_tile_kernels(row):
    """po2q_qconv2d_fused_f32 on plans whose kernel cannot apply the epilogue in its stores: the conv, then one
    elementwise pass (float4 where PQ % 4 == 0, scalar elsewhere), against oracle conv + numpy fp64 epilogue."""
    index, _ = T.find_plan(row)
    _check_fused(row[0], index, T.row_env(row), "auto", 31)


@pytest.mark.parametrize("row", T.FUSED_MFMA_ROWS, ids=["x".join(map(str, r[0])) for r in T.FUSED_MFMA_ROWS])
def test_fused_entry_on_the_fp32_mfma_kernel(row):
    assert T.describe(row[0], precision=row[1]).startswith("kind=mfma_f32 ")
    _check_fused(row[0], None, None, row[1], 32)


@pytest.mark.parametrize("shape", T.FUSED_DEPTHWISE_ROWS, ids=["x".join(map(str, s)) for s in T.FUSED_DEPTHWISE_ROWS])
def test_fused_entry_on_the_legacy_depthwise_kernel(shape):
    """conv_depthwise<true>: the whole epilogue in the kernel's own store."""
    assert T.describe(shape).startswith("kind=depthwise CC=1 NT=0 MI=1 NJ=1 vr=0 ")
    _check_fused(shape, None, None, "auto", 33)


def _octave_weights(shape, seed):
    g13, groups = T.geom(shape)
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(g13[4], g13[1] // groups, g13[5], g13[6], generator=g)
    return w * torch.exp2(torch.rand(w.shape, generator=g) * -40.0)


@pytest.mark.parametrize("row", T.WINDOW_ROWS, ids=[T.row_id(r) for r in T.WINDOW_ROWS])
def test_exponent_window(row):
    """bits 1, 2 and 7 and fsr = 2 with weight magnitudes spread over 40 octaves, so the clamp at the bottom of
    the exponent window [fsr - 2^(bits-1), fsr - 1] is exercised (at bits = 7 down to 2^-63 of the scale)."""
    shape = row[0]
    x, _, b = T.inputs(shape, 5)
    w = _octave_weights(shape, 6)
    xd, wd, bd = _dev(x, w, b)
    for bits, fsr in ((1, 1), (2, 1), (7, 1), (4, 2)):
        for mode in MODES:
            found = T.find_plan(row, mode, bits, fsr)
            assert found is not None, (bits, fsr, mode)
            ref = T.with_bias(T.reference(x, w, shape, mode, bits, fsr), b)
            y = T.run_plan(found[0], xd, wd, bd, shape, T.row_env(row), mode, bits, fsr).cpu().numpy()
            err = normwise_err(y, ref)
            assert err <= CONV_TOL, (bits, fsr, mode, err)


def test_bits_8_runs_the_fp32_mfma_kernel():
    """bits = 8: the window reaches 2^-127, no normal bf16, so precision auto plans mfma_f32 -- at the same bar."""
    for row in T.WINDOW_ROWS:
        shape = row[0]
        x, _, b = T.inputs(shape, 8)
        w = _octave_weights(shape, 9)
        xd, wd, bd = _dev(x, w, b)
        for mode in MODES:
            assert T.describe(shape, mode=mode, bits=8).startswith("kind=mfma_f32 ")
            ref = T.with_bias(T.reference(x, w, shape, mode, 8), b)
            y = T.run_plan(0, xd, wd, bd, shape, None, mode, 8).cpu().numpy()
            assert normwise_err(y, ref) <= CONV_TOL, (shape, mode, normwise_err(y, ref))


def _check_nonfinite(shape, index, env, precision):
    g13, _ = T.geom(shape)
    x = nonfinite_input(*g13[:4], sum(g13))
    _, w, _ = T.inputs(shape, 3)
    ref = torch.from_numpy(T.reference(x, w, shape, "po2")).float()
    fin = torch.isfinite(ref)
    assert (~fin).any() and fin.any()
    xd, wd = _dev(x, w)
    y = T.run_plan(index, xd, wd, None, shape, env, "po2", precision=precision).cpu()
    assert same_nonfinite(y, ref), (shape, int((torch.isnan(y) != torch.isnan(ref)).sum()),
                                    int((torch.isinf(y) != torch.isinf(ref)).sum()))
    err = ((y[fin] - ref[fin]).abs().max() / ref[fin].abs().max()).item()
    assert err <= CONV_TOL, (shape, err)


@pytest.mark.parametrize("row", T.NONFINITE_TILE_ROWS, ids=[T.row_id(r) for r in T.NONFINITE_TILE_ROWS])
def test_nonfinite_inputs_on_general_tap_tile_plans(row):
    """+-inf, NaN and a signalling NaN in x: exactly the oracle's NaN / +-inf pattern (padded k-slots and padded
    channels must contribute 0, never 0 * inf), finite outputs at the bar."""
    _check_nonfinite(row[0], T.find_plan(row)[0], T.row_env(row), "auto")


@pytest.mark.parametrize("row", T.NONFINITE_MFMA_ROWS, ids=["x".join(map(str, r[0])) for r in T.NONFINITE_MFMA_ROWS])
def test_nonfinite_inputs_on_the_fp32_mfma_kernel(row):
    _check_nonfinite(row[0], 0, None, row[1])


SENTINEL = -12345.678
GUARD = 256  # floats on either side of y


def _check_neighbours(shape, index, env, precision):
    """x is image 1 of a batch whose images 0 and 2 are all NaN; y sits in the middle of a sentinel-filled buffer."""
    g13, _ = T.geom(shape)
    x, w, b = T.inputs(shape, 21)
    big = torch.full((3,) + tuple(x.shape[1:]), float("nan"))
    big[1] = x[0]
    xd = big.to(DEV)[1:2]
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 0
    wd, bd = _dev(w, b)
    P, Q = T.out_size(shape)
    n = g13[4] * P * Q
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    y = buf[GUARD:GUARD + n].view(1, g13[4], P, Q)
    T.run_plan(index, xd, wd, bd, shape, env, "po2+", precision=precision, y=y)
    torch.cuda.synchronize()
    out = y.cpu()
    assert torch.isfinite(out).all(), "a read left the image: %d non-finite outputs" % int((~torch.isfinite(out)).sum())
    ref = T.with_bias(T.reference(x, w, shape, "po2+"), b)
    assert normwise_err(out.numpy(), ref) <= CONV_TOL, normwise_err(out.numpy(), ref)
    guard = torch.full((GUARD,), SENTINEL)
    assert torch.equal(buf[:GUARD].cpu(), guard), "a store landed before y"
    assert torch.equal(buf[GUARD + n:].cpu(), guard), "a store landed after y"


@pytest.mark.parametrize("row", T.NEIGHBOUR_TILE_ROWS, ids=[T.row_id(r) for r in T.NEIGHBOUR_TILE_ROWS])
def test_neighbouring_memory_tile_kernels(row):
    """C = 6 < CC with padding on all four sides: the channel tail and the halo come from the buffer range check
    (and the staging bounds), never from the NaN images around x; no store leaves y."""
    _check_neighbours(row[0], T.find_plan(row, "po2+")[0], T.row_env(row), "auto")


def test_neighbouring_memory_fp32_mfma_kernel():
    shape, prec, key = T.NEIGHBOUR_MFMA
    assert T.instance_key(T.parse(T.describe(shape, mode="po2+", precision=prec))) == key
    _check_neighbours(shape, 0, None, prec)


def test_neighbouring_memory_legacy_depthwise_kernel():
    assert T.describe(T.NEIGHBOUR_DEPTHWISE, mode="po2+").startswith("kind=depthwise CC=1 NT=0 MI=1 NJ=1 vr=0 ")
    _check_neighbours(T.NEIGHBOUR_DEPTHWISE, 0, None, "auto")


@pytest.mark.parametrize("row", T.ALIGNED_ROWS, ids=[T.row_id(r) + "-" + "".join(map(str, r[2])) for r in T.ALIGNED_ROWS])
def test_dword_aligned_views(row):
    """x and y each 4 bytes into their allocations, on vec = 1 plans (float4 epilogue stores; for the DMA kernel
    16-byte `buffer_load_dwordx4 ... lds` loads of x).

    Both kernels tolerate this, so the test asserts parity (and, the plan being the same, the bits of the run on
    16-byte aligned pointers) rather than a host-side choice of a scalar path:
      * Neither kernel dereferences a C++ float4 pointer for x or y.  The epilogue's store_f4 is inline
        `global_store_dwordx4`, the register-staged kernel reads x with raw 32-bit buffer loads, and the DMA kernel
        with inline `buffer_load_dwordx4 ... offen lds`; so no compiler alignment assumption is involved (unlike
        conv_dw3, whose float4 loads and stores are C++ vector accesses, which is why launch_conv_dw3 tests its
        pointers).
      * gfx9-family global and buffer memory instructions of 2 dwords or more need dword alignment only: the
        address unit splits them into dword requests, and the driver runs compute queues in the unaligned access
        mode in which the address is not forced down to the access size.  The buffer range check works on the
        byte offset against num_records, which the kernels set from the channel count, not from the base address.
      * The 16-byte requirement of LDS-DMA is on the LDS side (M0 + 16 * lane): lds_base, raw_off and the wave's
        1 KiB slots are multiples of 16 whatever x's address is (the CDNA guide's Guideline 17 concerns the
        dynamic-LDS base, not the global source).
      * The DMA kernel's 16-byte chunks never straddle an image row: W % 4 == 0 and the window starts d0 floats
        left of w0 at a multiple of 4 floats *relative to the row*, so a chunk is wholly inside or wholly outside
        the row for any base address."""
    shape = row[0]
    index, p = T.find_plan(row)
    P, Q = T.out_size(shape)
    assert Q % 4 == 0 and p.TQ % 4 == 0
    x, w, b = T.inputs(shape, 13)
    wd, bd = _dev(w, b)
    xbuf = torch.empty(x.numel() + 1, device=DEV)
    xs = xbuf[1:].view(x.shape)
    xs.copy_(x)
    ybuf = torch.zeros(shape[0] * shape[4] * P * Q + 1, device=DEV)
    ys = ybuf[1:].view(shape[0], shape[4], P, Q)
    assert xs.data_ptr() % 16 == 4 and ys.data_ptr() % 16 == 4
    T.run_plan(index, xs, wd, bd, shape, T.row_env(row), "po2", y=ys)
    ref = T.with_bias(T.reference(x, w, shape, "po2"), b)
    err = normwise_err(ys.cpu().numpy(), ref)
    assert err <= CONV_TOL, err
    ya = T.run_plan(index, x.to(DEV), wd, bd, shape, T.row_env(row), "po2")
    assert torch.equal(ys, ya)
    assert ybuf[0].item() == 0.0
