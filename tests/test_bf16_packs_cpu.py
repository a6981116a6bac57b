"""CPU: the batched weight staging of the bf16 conv forward (po2q_qconv2d_bf16_pack_batch +
po2q_qconv2d_packed_bf16) is exported, validates every job on the host before any launch with the
codes of the unbatched entry, has Meta kernels, and leaves CPU models alone."""
import ctypes

import pytest
import torch

from po2_quantization_amd import _lib
from po2_quantization_amd.models import quantized_conv as qc
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.utils.quantizers import quantizer_dict
from tests import _bf16_cases as cases

GEOM = dict(N=2, C=16, H=10, W=10, K=16, R=3, S=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, g=1)
ORDER = ("N", "C", "H", "W", "K", "R", "S", "sh", "sw", "ph", "pw", "dh", "dw", "g")
PTR = 16  # a dummy non-null pointer: every call here must return before anything is launched


def geom(over=None):
    a = dict(GEOM)
    a.update(over or {})
    return [a[k] for k in ORDER]


def call(L, over=None, mode=1, ws_bytes=1 << 20, ptr=PTR, bits=4):
    """The unbatched entry on dummy pointers, as tests/test_bf16_conv_cpu.py calls it."""
    p = ctypes.c_void_p(ptr)
    return L.po2q_qconv2d_bf16(p, p, None, p, *geom(over), bits, 1, mode, p, ws_bytes, None)


GOOD = dict(over=None, mode=1, bits=4, ptr=PTR, ws_bytes=1 << 20)


def pack_batch(L, jobs):
    """po2q_qconv2d_bf16_pack_batch of jobs = [dict(over=, mode=, bits=, ptr=, ws_bytes=, geom14=)]."""
    n = len(jobs)
    g = []
    for j in jobs:
        g += list(j.get("geom14") or geom(j["over"]))
    arr = lambda t, v: (t * max(len(v), 1))(*v)  # noqa: E731
    return L.po2q_qconv2d_bf16_pack_batch(
        n, arr(ctypes.c_void_p, [j["ptr"] for j in jobs]), arr(ctypes.c_int64, g),
        arr(ctypes.c_int, [j["bits"] for j in jobs]), arr(ctypes.c_int, [1] * n),
        arr(ctypes.c_int, [j["mode"] for j in jobs]), arr(ctypes.c_void_p, [j["ptr"] for j in jobs]),
        arr(ctypes.c_size_t, [j["ws_bytes"] for j in jobs]), None)


def test_symbols_exported():
    L = _lib.load()
    for name in ("po2q_qconv2d_bf16_pack_batch", "po2q_qconv2d_packed_bf16"):
        assert hasattr(L, name) and name in _lib.EXPORTS


BAD_JOBS = {
    "lin": dict(mode=3),
    "groups=2": dict(over={"g": 2}),
    "depthwise 7x7": dict(over={"g": 16, "R": 7, "S": 7, "ph": 3, "pw": 3}),
    "too large for LDS": dict(geom14=cases.geom14(cases.TOO_LARGE)),
    "bits=0": dict(bits=0),
    "null weight": dict(ptr=0),
    "workspace of 8 bytes": dict(ws_bytes=8),
}


@pytest.mark.parametrize("name", list(BAD_JOBS))
def test_batch_validates_every_job_before_any_launch(name):
    """A 3-job batch whose middle job is invalid returns what the unbatched entry returns for that job
    alone, names the job, and (the pointers being dummies) launches nothing."""
    L = _lib.load()
    bad = dict(GOOD, **BAD_JOBS[name])
    if "geom14" in bad:
        p = ctypes.c_void_p(PTR)
        alone = L.po2q_qconv2d_bf16(p, p, None, p, *bad["geom14"], 4, 1, 1, p, 1 << 20, None)
    else:
        alone = call(L, bad["over"], mode=bad["mode"], ws_bytes=bad["ws_bytes"], ptr=bad["ptr"], bits=bad["bits"])
    msg_alone = L.po2q_last_error()
    assert alone != 0
    assert pack_batch(L, [GOOD, bad, GOOD]) == alone
    msg = L.po2q_last_error()
    assert msg.startswith(msg_alone) and b"job 1" in msg, msg


def test_batch_expected_codes():
    L = _lib.load()
    code = lambda name: pack_batch(L, [GOOD, dict(GOOD, **BAD_JOBS[name]), GOOD])  # noqa: E731
    assert code("lin") == 2 and code("groups=2") == 2 and code("depthwise 7x7") == 2
    assert code("too large for LDS") == 1 and code("bits=0") == 1 and code("null weight") == 1
    assert code("workspace of 8 bytes") == 3


def test_empty_batch_is_ok():
    L = _lib.load()
    assert pack_batch(L, []) == 0
    assert L.po2q_qconv2d_bf16_pack_batch(0, None, None, None, None, None, None, None, None) == 0
    assert L.po2q_qconv2d_bf16_pack_batch(2, None, None, None, None, None, None, None, None) == 1
    assert L.po2q_qconv2d_bf16_pack_batch(-1, None, None, None, None, None, None, None, None) == 1


def packed(L, x=PTR, y=PTR, ws=PTR, ws_bytes=1 << 20, act=0, mode=1, over=None):
    p = lambda v: ctypes.c_void_p(v)  # noqa: E731
    return L.po2q_qconv2d_packed_bf16(p(x), None, p(y), *geom(over), 4, 1, mode, None, None, None, act, p(ws),
                                      ws_bytes, None)


def test_packed_entry_validation():
    L = _lib.load()
    assert packed(L, ws_bytes=8) == 3 and b"workspace" in L.po2q_last_error()
    for kw in (dict(x=0), dict(y=0), dict(ws=0)):
        assert packed(L, **kw) == 1 and b"null pointer" in L.po2q_last_error()
    assert packed(L, act=4) == 1 and b"activation" in L.po2q_last_error()
    assert packed(L, act=-1) == 1
    assert packed(L, mode=3) == 2 and packed(L, over={"g": 2}) == 2


def test_meta_kernels():
    _lib.ops()
    L = _lib.load()
    shapes = [cases.DENSE[2], cases.EDGES[1], cases.DEPTHWISE[0]]
    groups = [1, 1, cases.DEPTHWISE[0][1]]
    bits, modes = [4, 2, 8], [1, 2, 0]
    ws, geo = [], []
    for s, g in zip(shapes, groups):
        N, C, H, W, K, R, S = s[:7]
        ws.append(torch.empty(K, C // g, R, S, dtype=torch.bfloat16, device="meta"))
        geo += [N, C, H, W, *s[7:13], g]
    out = torch.ops.po2q.qconv2d_pack_batch_bf16(ws, geo, bits, modes, [1, 1, 1])
    assert len(out) == 3
    for t, s, g, b, m in zip(out, shapes, groups, bits, modes):
        need = L.po2q_qconv2d_bf16_workspace_bytes(*cases.geom14(s, g), b, 1, m)
        assert need > 0 and t.numel() == need and t.dtype == torch.uint8 and t.device.type == "meta"
    x = torch.empty(2, 16, 11, 15, dtype=torch.bfloat16, device="meta")
    w = torch.empty(24, 16, 3, 3, dtype=torch.bfloat16, device="meta")
    wsp = torch.empty(4096, dtype=torch.uint8, device="meta")
    y = torch.ops.po2q.qconv2d_packed_bf16(x, w, wsp, None, [2, 2], [1, 1], [1, 1], 1, 4, 1, 1, None, None, None, 1)
    assert tuple(y.shape) == (2, 24, 6, 8) and y.dtype == torch.bfloat16 and y.device.type == "meta"
    with pytest.raises(RuntimeError, match="lin"):
        torch.ops.po2q.qconv2d_pack_batch_bf16(ws[:1], geo[:11], [4], [3], [1])


def test_cpu_bf16_forward_opens_no_session(monkeypatch):
    torch.manual_seed(0)
    m = get_model("resnet20", 10, quantizer_dict["po2"], 4, (32, 32)).bfloat16().eval()
    x = torch.randn(2, 3, 32, 32).bfloat16()
    seen = []
    fwd = qc.QuantizedConv2d.forward
    monkeypatch.setattr(qc.QuantizedConv2d, "forward",
                        lambda self, inp: seen.append(getattr(qc._tls, "packs", None)) or fwd(self, inp))
    with torch.no_grad():
        monkeypatch.setattr(qc, "BATCHED_PACKS", False)
        ref = m(x)
        monkeypatch.setattr(qc, "BATCHED_PACKS", True)
        with qc.batched_packs(m, x):
            assert getattr(qc._tls, "packs", None) is None
        y1, y2 = m(x), m(x)
    assert seen and all(s is None for s in seen)
    assert torch.equal(y1, ref) and torch.equal(y2, ref)
    assert not qc._RECORDS.get(m)
