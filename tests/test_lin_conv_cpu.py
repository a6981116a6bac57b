"""CPU: the lin / lin+ conv modes on the host side -- planning, bf16x3 eligibility, workspace
sizes, the multi-layer entries' refusal, the quantizer entry's refusal and the Meta kernels.
No GPU work is started by these calls (host-only planning, as tests/test_capi.py)."""
import ctypes

import pytest
import torch

from po2_quantization_amd import _lib

NUM_ITERS = 10  # the `fsr` slot of the C ABI carries num_iters in the lin modes

# N, C, H, W, K, R, S, stride, padding, groups
PLAN_SHAPES = [
    (2, 16, 10, 12, 16, 3, 3, 1, 1, 1),
    (2, 32, 8, 8, 32, 3, 3, 1, 1, 1),
    (1, 64, 6, 8, 64, 3, 3, 1, 1, 1),
    (2, 96, 5, 5, 24, 1, 1, 1, 0, 1),    # 1x1 96 -> 24
    (2, 32, 8, 8, 32, 3, 3, 1, 1, 32),   # depthwise 32
]
ELIGIBLE = PLAN_SHAPES[:4]


def _plans(shape, mode, bits=4, iters=NUM_ITERS, precision="auto", groups=None):
    N, C, H, W, K, R, S, st, pad, g = shape
    return _lib.plans(N, C, H, W, K, R, S, st, pad, 1, g if groups is None else groups, bits, mode, iters, precision)


def _describe(shape, mode, bits=4, iters=NUM_ITERS, precision="auto", groups=None):
    N, C, H, W, K, R, S, st, pad, g = shape
    return _lib.describe(N, C, H, W, K, R, S, st, pad, 1, g if groups is None else groups, bits, mode, iters,
                         precision)


def _c_args(shape, groups=None):
    N, C, H, W, K, R, S, st, pad, g = shape
    return (N, C, H, W, K, R, S, st, st, pad, pad, 1, 1, g if groups is None else groups)


@pytest.mark.parametrize("mode", ["lin", "lin+"])
@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_lin_plans(shape, mode):
    ps = _plans(shape, mode)
    assert len(ps) >= 1
    assert ps[0] == _describe(shape, mode)
    for p in ps:
        assert " fp=1" not in p and "direct_f32" not in p and "pw_f32" not in p, p


@pytest.mark.parametrize("mode", ["lin", "lin+"])
@pytest.mark.parametrize("shape", ELIGIBLE)
def test_lin_eligible_shapes_take_bf16x3(shape, mode):
    assert "kind=bf16x3" in _describe(shape, mode)
    assert "kind=bf16x3" in _describe(shape, mode, bits=9, iters=1)
    assert "kind=bf16x3" in _describe(shape, mode, precision="bf16x3")


@pytest.mark.parametrize("over", [dict(bits=10), dict(iters=0), dict(groups=2)])
def test_lin_ineligible_problems_take_fp32_and_refuse_bf16x3(over):
    shape = PLAN_SHAPES[0]
    assert "kind=bf16x3" not in _describe(shape, "lin", **over)
    L = _lib.load()
    bits, iters = over.get("bits", 4), over.get("iters", NUM_ITERS)
    n = L.po2q_qconv2d_plans(*_c_args(shape, over.get("groups")), bits, iters, _lib.MODES["lin"],
                             _lib.PRECISIONS["bf16x3"], -1, None, 0)
    assert n == -2  # PO2Q_ERR_UNSUPPORTED
    assert b"bf16x3" in L.po2q_last_error()


def test_lin_rejects_negative_num_iters():
    L = _lib.load()
    n = L.po2q_qconv2d_plans(*_c_args(PLAN_SHAPES[0]), 4, -1, _lib.MODES["lin"], 0, -1, None, 0)
    assert n == -1  # PO2Q_ERR_INVALID
    assert b"num_iters" in L.po2q_last_error()


@pytest.mark.parametrize("mode", ["lin", "lin+"])
@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_lin_workspace_covers_the_steps(shape, mode):
    L = _lib.load()
    po2 = L.po2q_qconv2d_workspace_bytes(*_c_args(shape), 4, 1, _lib.MODES["po2"], 0)
    lin = L.po2q_qconv2d_workspace_bytes(*_c_args(shape), 4, NUM_ITERS, _lib.MODES[mode], 0)
    assert lin > 0
    assert lin >= po2


def test_po2_workspace_unchanged_by_the_lin_layout():
    """The delta[Cg] region exists in the lin modes only (po2 sizes as test_capi pins them)."""
    L = _lib.load()
    shape = PLAN_SHAPES[0]
    po2 = L.po2q_qconv2d_workspace_bytes(*_c_args(shape), 4, 1, _lib.MODES["po2"], 0)
    lin = L.po2q_qconv2d_workspace_bytes(*_c_args(shape), 4, NUM_ITERS, _lib.MODES["lin"], 0)
    assert 0 < lin - po2 <= 4096


@pytest.mark.parametrize("mode", ["lin", "lin+"])
def test_multi_layer_entries_refuse_lin(mode):
    assert _lib.pair_supported((256, 16, 224, 224), 4, "po2")
    assert not _lib.pair_supported((256, 16, 224, 224), 4, mode, NUM_ITERS)
    assert _lib.s2ds_supported((256, 32, 112, 112), 4, "po2")
    assert not _lib.s2ds_supported((256, 32, 112, 112), 4, mode, NUM_ITERS)
    assert _lib.chain_supported((8, 16, 32, 32), 6, 4, "po2")
    assert not _lib.chain_supported((8, 16, 32, 32), 6, 4, mode, NUM_ITERS)
    # a 4x4 MobileNetV2 block (96 -> 576 -> 96, stride 1)
    assert _lib.ir_shape_supported((8, 96, 4, 4), 576, 96, 1, True)
    assert not _lib.ir_shape_supported((8, 96, 4, 4), 576, 96, 1, True, mode=mode)
    # the C entries themselves, with the mode ids
    L = _lib.load()
    m = _lib.MODES[mode]
    assert L.po2q_qconv2d_pair_supported(256, 16, 224, 224, 4, NUM_ITERS, m) == 0
    assert L.po2q_qconv2d_s2ds_supported(256, 32, 112, 112, 4, NUM_ITERS, m) == 0
    assert L.po2q_qconv2d_chain_supported(8, 16, 32, 32, 6, 4, NUM_ITERS, m) == 0


def test_ir_supported_refuses_lin_plans():
    """po2q_qconv2d_ir_supported: 1 for the three po2 plans of a 4x4 block, 0 when any is a lin plan."""
    L = _lib.load()

    def plan(args, mode):
        h = ctypes.c_void_p()
        fsr = NUM_ITERS if mode != "po2" else 1
        assert L.po2q_qconv2d_plan_create(ctypes.byref(h), 0, *args, 4, fsr, _lib.MODES[mode], 0) == 0
        return h

    e_args = (8, 96, 4, 4, 576, 1, 1, 1, 1, 0, 0, 1, 1, 1)
    d_args = (8, 576, 4, 4, 576, 3, 3, 1, 1, 1, 1, 1, 1, 576)
    p_args = (8, 576, 4, 4, 96, 1, 1, 1, 1, 0, 0, 1, 1, 1)
    hs = []
    try:
        for modes in [("po2", "po2", "po2"), ("lin", "po2", "po2"), ("po2", "lin", "po2"), ("po2", "po2", "lin+"),
                      ("lin", "lin", "lin")]:
            e, d, p = plan(e_args, modes[0]), plan(d_args, modes[1]), plan(p_args, modes[2])
            hs += [e, d, p]
            assert L.po2q_qconv2d_ir_supported(e, d, p) == (1 if modes == ("po2", "po2", "po2") else 0), modes
    finally:
        for h in hs:
            L.po2q_qconv2d_plan_destroy(h)


def test_multi_layer_run_entries_refuse_lin_before_any_launch():
    L = _lib.load()
    p = ctypes.c_void_p(16)
    for m in (3, 4):
        assert L.po2q_qconv2d_pair_f32(p, p, p, p, 256, 16, 224, 224, 4, NUM_ITERS, m, None, None, None, None, 0,
                                       None, None, None, 0, None) == 2
        assert b"lin" in L.po2q_last_error()
        assert L.po2q_qconv2d_s2ds_f32(p, p, p, p, p, 256, 32, 112, 112, 4, NUM_ITERS, m, None, None, 0, None, None,
                                       None) == 2
        wa = (ctypes.c_void_p * 2)(16, 16)
        assert L.po2q_qconv2d_chain_f32(p, wa, None, None, None, None, None, 2, 8, 16, 32, 32, 4, NUM_ITERS, m, p, p,
                                        1 << 20, None) == 2


@pytest.mark.parametrize("mode_id", [3, 4])
def test_quantizer_entry_still_rejects_lin_modes(mode_id):
    L = _lib.load()
    dummy = ctypes.c_void_p(16)
    assert L.po2q_quantize_f32(dummy, dummy, 10, 4, 1, mode_id, dummy, 256, None) == 1  # PO2Q_ERR_INVALID
    assert b"mode" in L.po2q_last_error()


def test_python_quantize_rejects_lin_mode_strings():
    with pytest.raises(_lib.Po2qError, match="po2"):
        _lib.quantize(torch.zeros(4), 4, "lin")


@pytest.mark.parametrize("mode_id", [3, 4])
def test_meta_kernels_give_the_po2_shapes(mode_id):
    O = _lib.ops()
    x = torch.empty(2, 16, 10, 12, device="meta")
    w = torch.empty(24, 16, 3, 3, device="meta")
    for stride, pad in ((1, 1), (2, 0)):
        ref = O.qconv2d(x, w, None, [stride, stride], [pad, pad], [1, 1], 1, 4, 1, 1, 0, -1, 0)
        y = O.qconv2d(x, w, None, [stride, stride], [pad, pad], [1, 1], 1, 4, mode_id, NUM_ITERS, 0, -1, 0)
        assert y.shape == ref.shape and y.device.type == "meta"
        yf = O.qconv2d_fused(x, w, None, [stride, stride], [pad, pad], [1, 1], 1, 4, mode_id, NUM_ITERS, 0, -1, 0,
                             None, None, None, 1)
        assert yf.shape == ref.shape and yf.device.type == "meta"
