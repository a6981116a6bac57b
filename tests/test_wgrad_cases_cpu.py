"""CPU: the weight-gradient case tables (tests/_wgrad_cases.py) reach what they claim.  The host-only
po2q_qconv2d_wgrad_describe names the kernel and plan of each shape from the plan the launch itself
resolves; these tests fail, naming the instance or condition, when a table row or a planner
heuristic changes so that a kernel instance or a loop form is no longer run by the GPU tests."""
import ctypes
import itertools

import pytest

from po2_quantization_amd import _lib
from tests import _wgrad_cases as cases


def plans(shapes, groups=None):
    return [cases.parse(cases.describe(s, s[1] if groups == "dw" else 1)) for s in shapes]


def test_describe_lines():
    assert cases.describe(cases.LONG_RING) == ("kind=wgrad_stream R=3 SH=1 KW=2 CW=2 vec=1 RB=8 nseg=32 nstrip=1 "
                                               "items=128 bpg=32 KG=16 CG=2")
    assert cases.describe(cases.BAND[0]) == "kind=wgrad_band R=3 S=3 BP=5 XR=9 QT=64 nqt=2 WT=68 KT=3 CT=2 lds=59776"
    assert cases.describe(cases.DEPTHWISE[0], 8) == "kind=wgrad_dw RS=9 nslice=2 per_slice=5"


def test_describe_status_is_the_launch_status():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p(16)
    for shape, groups in [(cases.NO_PLAN_D6, 1), (cases.DEPTHWISE_UNSUPPORTED, 16), (cases.BAND[0], 2),
                          ((2, 16, 9, 9, 16, 5, 5, 1, 1, 2, 2, 1, 1), 1), ((2, 16, 9, 9, 16, 3, 3, 0, 1, 1, 1, 1, 1), 1)]:
        st = L.po2q_qconv2d_wgrad_describe(*shape, groups, buf, 256)
        msg = L.po2q_last_error()
        assert st != 0 and msg.startswith(b"po2q"), (shape, st, msg)
        # the launch validates the geometry before it touches a pointer: same status, same message
        assert L.po2q_qconv2d_wgrad_f32(p, p, p, *shape, groups, p, 1 << 20, None) == st, shape
        assert L.po2q_last_error() == msg, shape
    assert L.po2q_qconv2d_wgrad_describe(*cases.BAND[0], 1, None, 0) == 1
    assert L.po2q_qconv2d_wgrad_describe(*cases.BAND[0], 1, buf, 8) == 0 and buf.value == b"kind=wg"  # truncated


def test_stream_grid_is_exactly_the_32_instances():
    got = {}
    for shape in cases.STREAM_GRID:
        kind, f = cases.parse(cases.describe(shape))
        assert kind == "wgrad_stream", (shape, kind)
        got.setdefault((f["R"], f["SH"], f["KW"], f["CW"], f["vec"]), []).append(shape)
    want = set(itertools.product((3, 1), (1, 2), (1, 2), (1, 2), (1, 0)))
    missing = sorted(want - set(got))
    assert not missing, "wgrad2_f32 instances (R, SH, KW, CW, vec) no grid shape reaches: %s" % missing
    assert set(got) == want and len(cases.STREAM_GRID) == 32
    assert all(len(v) == 1 for v in got.values()), got


def test_tables_describe_as_their_kernel():
    for shape in cases.STREAM:
        assert cases.parse(cases.describe(shape))[0] == "wgrad_stream", shape
    for shape in cases.BAND:
        assert cases.parse(cases.describe(shape))[0] == "wgrad_band", shape
    for shape in cases.DEPTHWISE:
        assert cases.parse(cases.describe(shape, shape[1]))[0] == "wgrad_dw", shape
    for shape in cases.ALIGNMENT:
        assert shape in cases.STREAM_GRID and cases.parse(cases.describe(shape))[1]["vec"] == 1, shape
    for shape, groups in cases.RUN:
        assert cases.exact_sums_fit(shape), shape


def _long(f, P):
    return f["RB"] > 4 and f["nseg"] > 1 and P % f["RB"] != 0


CONDITIONS = {
    # register-streaming kernel: segments longer than one turn of the row loop, ragged last segment
    "stream: RB > 4, nseg > 1, P % RB != 0 in the 4-slot ring (3x3 stride 1)":
        lambda: any(f["R"] == 3 and f["SH"] == 1 and _long(f, cases.out_size(s)[0])
                    for s, (_, f) in zip(cases.STREAM, plans(cases.STREAM))),
    "stream: RB > 4, nseg > 1, P % RB != 0 in the two-slot loop (3x3 stride 2)":
        lambda: any(f["R"] == 3 and f["SH"] == 2 and _long(f, cases.out_size(s)[0])
                    for s, (_, f) in zip(cases.STREAM, plans(cases.STREAM))),
    "stream: RB > 4, nseg > 1, P % RB != 0 in the 1x1 form":
        lambda: any(f["R"] == 1 and _long(f, cases.out_size(s)[0])
                    for s, (_, f) in zip(cases.STREAM, plans(cases.STREAM))),
    "stream: bpg > 16 (wgrad2_reduce's slice loop runs more than once)":
        lambda: any(f["bpg"] > 16 for _, f in plans(cases.STREAM)),
    "stream: items % 4 != 0 (a block with idle waves)":
        lambda: any(f["items"] % 4 != 0 for _, f in plans(cases.STREAM)),
    "band: nqt > 1": lambda: any(f["nqt"] > 1 for _, f in plans(cases.BAND)),
    "band: BP == 1": lambda: any(f["BP"] == 1 for _, f in plans(cases.BAND)),
    "band: P % BP != 0": lambda: any(cases.out_size(s)[0] % f["BP"] != 0
                                     for s, (_, f) in zip(cases.BAND, plans(cases.BAND))),
    "band: R == 1": lambda: any(f["R"] == 1 for _, f in plans(cases.BAND)),
    "band: sh != sw": lambda: any(s[7] != s[8] for s in cases.BAND),
    "band: last column tile ragged and not a multiple of 4 wide":
        lambda: any(f["nqt"] > 1 and (cases.out_size(s)[1] % f["QT"]) % 4 != 0
                    for s, (_, f) in zip(cases.BAND, plans(cases.BAND))),
    "band: K and C not multiples of 16":
        lambda: any(s[4] % 16 and s[1] % 16 for s in cases.BAND),
    "depthwise: nslice > 1 with N % per_slice != 0":
        lambda: any(f["nslice"] > 1 and s[0] % f["per_slice"] != 0
                    for s, (_, f) in zip(cases.DEPTHWISE, plans(cases.DEPTHWISE, "dw"))),
    "depthwise: RS == 25 with R != S":
        lambda: any(f["RS"] == 25 and s[5] != s[6]
                    for s, (_, f) in zip(cases.DEPTHWISE, plans(cases.DEPTHWISE, "dw"))),
    "depthwise: P * Q below one block":
        lambda: any(cases.out_size(s)[0] * cases.out_size(s)[1] < 256 for s in cases.DEPTHWISE),
}


@pytest.mark.parametrize("name", list(CONDITIONS))
def test_condition_is_reached(name):
    assert CONDITIONS[name](), "no case reaches: " + name


def test_no_plan_cases():
    L = _lib.load()
    for shape in cases.NO_PLAN:
        with pytest.raises(_lib.Po2qError, match="no plan fits"):
            cases.describe(shape)
        assert L.po2q_qconv2d_wgrad_workspace_bytes(*shape, 1) == 0
        stride, pad, dil = cases.conv_args(shape)
        assert _lib.wgrad_supported(cases.wshape(shape), 1)  # the weight shape alone is a native one
        assert not _lib.wgrad_supported(cases.wshape(shape), 1, shape[:4], stride, pad, dil)
    with pytest.raises(_lib.Po2qError, match="depthwise wgrad: unsupported"):
        cases.describe(cases.DEPTHWISE_UNSUPPORTED, 16)
    assert L.po2q_qconv2d_wgrad_workspace_bytes(*cases.DEPTHWISE_UNSUPPORTED, 16) == 0


def test_wgrad_supported_with_geometry():
    for shape, groups in cases.RUN:
        stride, pad, dil = cases.conv_args(shape)
        assert _lib.wgrad_supported(cases.wshape(shape, groups), groups, shape[:4], stride, pad, dil), shape
    # the two-argument form looks at the weight shape only, as before
    assert _lib.wgrad_supported((16, 16, 3, 3), 1) and _lib.wgrad_supported((8, 1, 5, 5), 8)
    assert not _lib.wgrad_supported((16, 16, 5, 5), 1) and not _lib.wgrad_supported((16, 8, 3, 3), 2)
    assert not _lib.wgrad_supported((16, 16, 5, 5), 1, (2, 16, 9, 9), 1, 2, 1)
