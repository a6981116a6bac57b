"""CPU: the bf16 conv entries (po2q_qconv2d_bf16*) are exported, validate on the host before any
launch, describe their kernels, have a Meta kernel, and leave CPU modules on the torch path."""
import ctypes

import pytest
import torch

from po2_quantization_amd import _lib, ptq
from po2_quantization_amd.models.quantized_conv import QuantizedConv2d
from po2_quantization_amd.utils.quantizers import quantizer_dict
from tests import _bf16_cases as cases

GEOM = dict(N=2, C=16, H=10, W=10, K=16, R=3, S=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, g=1)
ORDER = ("N", "C", "H", "W", "K", "R", "S", "sh", "sw", "ph", "pw", "dh", "dw", "g")


def geom(over=None):
    a = dict(GEOM)
    a.update(over or {})
    return [a[k] for k in ORDER]


def call(L, over=None, mode=1, ws_bytes=1 << 20, ptr=16, bits=4):
    p = ctypes.c_void_p(ptr)
    return L.po2q_qconv2d_bf16(p, p, None, p, *geom(over), bits, 1, mode, p, ws_bytes, None)


def test_symbols_exported():
    L = _lib.load()
    for name in ("po2q_qconv2d_bf16_workspace_bytes", "po2q_qconv2d_bf16", "po2q_qconv2d_bf16_describe"):
        assert hasattr(L, name) and name in _lib.EXPORTS


def test_host_validation():
    L = _lib.load()
    assert call(L, mode=3) == 2 and b"lin" in L.po2q_last_error()
    assert call(L, mode=4) == 2
    assert call(L, mode=9) == 1 and b"mode" in L.po2q_last_error()
    assert call(L, bits=0) == 1 and b"bits" in L.po2q_last_error()
    assert call(L, {"g": 2}) == 2 and b"groups" in L.po2q_last_error()  # grouped, not depthwise
    assert call(L, {"g": 16, "R": 7, "S": 7, "ph": 3, "pw": 3}) == 2    # depthwise beyond 5x5
    assert call(L, ws_bytes=8) == 3
    assert call(L, ptr=0) == 1 and b"null pointer" in L.po2q_last_error()
    assert L.po2q_qconv2d_bf16_workspace_bytes(*geom(), 4, 1, 1) > 0
    assert L.po2q_qconv2d_bf16_workspace_bytes(*geom(), 4, 1, 3) == 0
    assert L.po2q_qconv2d_bf16_workspace_bytes(*geom({"g": 2}), 4, 1, 1) == 0


@pytest.mark.parametrize("over,msg", [
    ({"C": 15, "g": 2}, b"divisible by groups"),
    ({"H": 1, "ph": 0}, b"kernel size"),
    ({"sh": 0}, b"stride"),
    ({"N": 0}, b"positive"),
])
def test_geometry_messages_of_the_fp32_entry(over, msg):
    L = _lib.load()
    assert call(L, over) == 1
    assert msg in L.po2q_last_error()
    p = ctypes.c_void_p(16)
    a = dict(GEOM)
    a.update(over)
    assert L.po2q_qconv2d_f32(p, p, None, p, *[a[k] for k in ORDER], 4, 1, 1, 0, p, 1 << 20, None) == 1
    assert msg in L.po2q_last_error()


def test_describe():
    assert _lib.describe_bf16(2, 16, 10, 10, 16, 3, 3, 1, 1).startswith("kind=bf16x1 ")
    assert _lib.describe_bf16(256, 16, 224, 224, 16, 3, 3, 1, 1).startswith("kind=bf16x1 ")
    assert _lib.describe_bf16(2, 24, 9, 9, 24, 3, 3, 1, 1, groups=24).startswith("kind=dw_bf16 ")
    with pytest.raises(_lib.Po2qError, match="lin"):
        _lib.describe_bf16(2, 16, 10, 10, 16, 3, 3, 1, 1, mode="lin")


def test_meta_kernel():
    _lib.ops()
    x = torch.empty(2, 16, 11, 15, dtype=torch.bfloat16, device="meta")
    w = torch.empty(24, 16, 3, 3, dtype=torch.bfloat16, device="meta")
    y = torch.ops.po2q.qconv2d_bf16(x, w, None, [2, 2], [1, 1], [1, 1], 1, 4, 1, 1)
    assert tuple(y.shape) == (2, 24, 6, 8) and y.dtype == torch.bfloat16 and y.device.type == "meta"


def test_cpu_bf16_module_takes_the_torch_path():
    torch.manual_seed(0)
    conv = QuantizedConv2d(4, 6, 3, quantize_fn=quantizer_dict["po2"], bits=4).bfloat16()
    x = torch.randn(1, 4, 8, 8).bfloat16()
    ref = torch.nn.functional.conv2d(x, _lib.restated_quantize(conv.weight.detach(), 4, "po2"), None, 1, 1)
    y = conv(x)  # grad mode on: the CPU path keeps the reference's autograd behaviour
    assert y.dtype == torch.bfloat16 and y.requires_grad and torch.equal(y.detach(), ref)
    with pytest.raises(_lib.Po2qError, match="HIP device"):
        _lib.qconv2d_bf16(x, conv.weight.detach(), None, 1, 1)


def test_ptq_dtype_option():
    ap = ptq.arg_parser()
    base = ["resnet20", "cifar", "--data_file", "x.pt"]
    assert ap.parse_args(base).dtype == "fp32"
    assert ap.parse_args(base + ["--dtype", "bf16"]).dtype == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--dtype", "fp16"])
    assert ptq.DTYPES["bf16"] == torch.bfloat16


# ---- coverage of the bf16 kernel family by the shared case table (tests/_bf16_cases.py) --------
# Set-level conditions, not per-shape equalities: a planner retune fails these only when an
# instance or a path is no longer reached by any shape tests/test_gpu_bf16_conv_paths.py runs.
def _plans():
    return [(s, cases.parse_plan(d), cases.parse_lds(d)) for s, d in ((s, cases.describe(s)) for s in cases.DENSE)]


def test_case_table_reaches_every_instance():
    reached = {(p.CC, p.NT, p.NJ) for _, p, _ in _plans()}
    every = {(cc, nt, nj) for cc in (16, 32) for nt in (1, 2, 4) for nj in (1, 2, 4)}
    missing = sorted(every - reached)
    print("instances reached: %d of %d" % (len(reached & every), len(every)))
    assert not missing, "no dense case reaches conv_bf16x1<CC, NT, NJ> for %s" % missing
    assert reached == every, "instances outside the template grid: %s" % sorted(reached - every)


CONDITIONS = {  # name -> predicate of (shape, plan, LDS bytes)
    "kblocks > 1 together with chunks > 1": lambda s, p, lds: p.kblocks > 1 and p.chunks > 1,
    "TQ % 4 != 0 (2-byte epilogue only)": lambda s, p, lds: p.TQ % 4 != 0,
    "ksteps >= 13 with K > 16 and NT = 1 (NT halved to fit LDS)":
        lambda s, p, lds: p.ksteps >= 13 and s[4] > 16 and p.NT == 1,
    "tilesP > 1 and tilesQ > 1 with W even (pair staging)":
        lambda s, p, lds: p.tilesP > 1 and p.tilesQ > 1 and s[3] % 2 == 0,
    "tilesP > 1 and tilesQ > 1 with W odd (2-byte staging)":
        lambda s, p, lds: p.tilesP > 1 and p.tilesQ > 1 and s[3] % 2 == 1,
    "lds > 48 KiB": lambda s, p, lds: lds > 48 * 1024,
}


def test_case_table_meets_every_named_condition():
    plans = _plans()
    unmet = [name for name, cond in CONDITIONS.items() if not any(cond(s, p, lds) for s, p, lds in plans)]
    for name, cond in CONDITIONS.items():
        print("%s: %s" % (name, [cases.case_id(s) for s, p, lds in plans if cond(s, p, lds)]))
    assert not unmet, "no dense case meets: %s" % unmet


def test_alignment_cases_cover_both_stagings_and_both_stores():
    seen = {(s[3] % 2 == 0, cases.parse_plan(cases.describe(s)).TQ % 4 == 0) for s in cases.ALIGNMENT}
    missing = {(pair, vec) for pair in (True, False) for vec in (True, False)} - seen
    assert not missing, "no alignment case has (pair staging, 8-byte stores) = %s" % sorted(missing)


def test_depthwise_cases_run_the_depthwise_kernel():
    for s in cases.DEPTHWISE:
        assert cases.describe(s, groups=s[1]).startswith("kind=dw_bf16 "), s


def test_too_large_kernel_is_refused_on_the_host():
    with pytest.raises(_lib.Po2qError, match="LDS"):
        cases.describe(cases.TOO_LARGE)
    L = _lib.load()
    for mode in (0, 1, 2):
        assert L.po2q_qconv2d_bf16_workspace_bytes(*cases.geom14(cases.TOO_LARGE), 4, 1, mode) == 0
    assert cases.describe(cases.LARGEST).startswith("kind=bf16x1 ")  # 9x9 is the largest that fits
