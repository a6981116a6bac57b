"""GPU parity of the pipelined conv-1 schedule of the role-split conv pairs: the conv-1 waves issue their
vector work (epilogue 1, the exact split of the next x row; in conv_pair64 the x DMAs too) in slices
between their own MFMAs, conv_pairw splitting one row ahead into a second plane set per strip.  Same
fragments, same MFMA order per accumulator, same epilogue expressions (two chained
QuantizedConv2d.forward calls, reference models/quantized_conv.py:32-38; the BasicBlock epilogues of
models/resnet.py:55-71), so every output is bit for bit the earlier schedule's, which stays in the build
(PO2Q_PAIR_W32_PIPE=0 / PO2Q_PAIR64_PIPE=0), and
  conv_pairw (C = 32):  the 7-wave conv_pair<32>'s (PO2Q_PAIR_W32=0), and within CONV_TOL (normwise 1e-5) of
                        the reference's CPU path; the residual forms keep the earlier schedule;
  conv_pair64:          two conv_rowsk launches'; images shorter than conv_rowsk's smallest plan are held
                        to the oracle bar."""
import functools
import math

import pytest
import torch

from oracle import oracle as O
from po2_quantization_amd import _lib
from tests._nonfinite import same_nonfinite
from tests._util import CONV_TOL, normwise_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "PO2Q_PAIR64_PIPE"

WS = (36, 48, 52, 56, 64)
# H + 6 steps: 4, 6 / 7, 12 / 13 land on both sides of the 6-step unroll's break; W = 36 / 48: the
# 3-group kernel, 52 / 56: a partly filled last group, 64: the full width
BIT_SHAPES = [(2, h, w) for h in (4, 6, 7, 12, 13) for w in WS]
# shorter than the pipeline's fill: every step but a few skips its MFMAs and runs the slices serially
SHORT_SHAPES = [(2, h, w) for h in (1, 2, 3) for w in WS]


def kaiming(gen, C=64):
    return torch.randn(C, C, 3, 3, generator=gen) * math.sqrt(2.0 / (C * 9))


@functools.lru_cache(maxsize=None)
def case(N, H, W):
    g = torch.Generator().manual_seed(7000 + 100 * H + W)
    x = torch.randn(N, 64, H, W, generator=g)
    return x, kaiming(g), kaiming(g)


@functools.lru_cache(maxsize=None)
def reference(N, H, W, mode):
    x, w1, w2 = case(N, H, W)
    h = O.cpu_reference_qconv2d(x, w1, None, 1, 1, 1, 1, 4, mode)
    return O.cpu_reference_qconv2d(h, w2, None, 1, 1, 1, 1, 4, mode).numpy()


def rowsk_plan(N, H, W, mode):
    """Index of a conv_rowsk candidate (packed weights, temporal loads / stores), or None."""
    for i, d in enumerate(_lib.plans(N, 64, H, W, 64, 3, 3, 1, 1, 1, 1, 4, mode)):
        if "kind=bf16x3_rows " in d and " fp=0" in d and " nts=0 " in d and (" vr=1 " in d or " vr=2 " in d):
            return i
    return None


def two_singles(x, w1, w2, mode, plan):
    h = _lib.qconv2d(x, w1, None, 1, 1, 1, 1, 4, mode, plan=plan)
    return _lib.qconv2d(h, w2, None, 1, 1, 1, 1, 4, mode, plan=plan)


def both_schedules(monkeypatch, fn):
    """fn() under the earlier schedule and under the pipelined one (the default)."""
    monkeypatch.setenv(KNOB, "0")
    old = fn()
    monkeypatch.setenv(KNOB, "1")
    new = fn()
    monkeypatch.delenv(KNOB)
    return old, new, fn()


@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=[str(s) for s in BIT_SHAPES])
def test_pair64_pipelined_bit_for_bit(shape, mode, monkeypatch):
    x, w1, w2 = (t.to(DEV) for t in case(*shape))
    old, new, default = both_schedules(monkeypatch, lambda: _lib.qconv2d_pair(x, w1, w2, 4, mode))
    plan = rowsk_plan(*shape, mode)
    assert plan is not None
    ref = two_singles(x, w1, w2, mode, plan)
    print("pair64 pipelined", shape, mode, "differing elements: vs old %d, vs 2 x conv_rowsk %d"
          % (int((new != old).sum()), int((new != ref).sum())))
    assert torch.isfinite(new).all() and float(new.abs().max()) > 0
    assert torch.equal(new, old)
    assert torch.equal(new, ref)
    assert torch.equal(default, new)  # on by default


@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("shape", SHORT_SHAPES, ids=[str(s) for s in SHORT_SHAPES])
def test_pair64_pipelined_short_images_vs_oracle(shape, mode, monkeypatch):
    x, w1, w2 = (t.to(DEV) for t in case(*shape))
    old, new, _ = both_schedules(monkeypatch, lambda: _lib.qconv2d_pair(x, w1, w2, 4, mode))
    err = normwise_err(new.cpu().numpy(), reference(*shape, mode))
    print("pair64 pipelined", shape, mode, "normwise err %.3g" % err)
    assert err <= CONV_TOL, err
    assert torch.equal(new, old)


def test_pair64_pipelined_bias(monkeypatch):
    shape = (2, 7, 52)
    x, w1, w2 = (t.to(DEV) for t in case(*shape))
    g = torch.Generator().manual_seed(3)
    b1, b2 = (torch.randn(64, generator=g) * 0.1).to(DEV), (torch.randn(64, generator=g) * 0.1).to(DEV)
    old, new, _ = both_schedules(monkeypatch, lambda: _lib.qconv2d_pair(x, w1, w2, 4, "po2", bias1=b1, bias2=b2))
    plan = rowsk_plan(*shape, "po2")
    h = _lib.qconv2d(x, w1, b1, 1, 1, 1, 1, 4, "po2", plan=plan)
    assert torch.equal(new, old)
    assert torch.equal(new, _lib.qconv2d(h, w2, b2, 1, 1, 1, 1, 4, "po2", plan=plan))


@pytest.mark.parametrize("mode", ["po2", "po2+"])
def test_pair64_pipelined_row_segments(mode, monkeypatch):
    """Two row segments: the split one row ahead and the deferred epilogue 1 cross a segment's halo."""
    shape = (2, 9, 56)
    x, w1, w2 = (t.to(DEV) for t in case(*shape))
    one = _lib.qconv2d_pair(x, w1, w2, 4, mode)
    monkeypatch.setenv("PO2Q_PAIR64_NSEG", "2")
    old, new, _ = both_schedules(monkeypatch, lambda: _lib.qconv2d_pair(x, w1, w2, 4, mode))
    assert torch.equal(new, old)
    assert torch.equal(new, one)
    assert torch.equal(new, two_singles(x, w1, w2, mode, rowsk_plan(*shape, mode)))


def test_pair64_pipelined_nonfinite_inputs(monkeypatch):
    """+-inf and NaN in the first and last image row and in the last valid column propagate as they do
    through the earlier schedule and through two single calls, NaNs in the same places."""
    shape = (2, 7, 52)
    x, w1, w2 = case(*shape)
    x = x.clone()
    x[0, 3, 0, 10] = float("inf")
    x[0, 40, 6, 51] = float("-inf")
    x[1, 17, 6, 0] = float("nan")
    x[1, 63, 0, 51] = float("nan")
    xd, w1d, w2d = x.to(DEV), w1.to(DEV), w2.to(DEV)
    old, new, _ = both_schedules(monkeypatch, lambda: _lib.qconv2d_pair(xd, w1d, w2d, 4, "po2"))
    ref = two_singles(xd, w1d, w2d, "po2", rowsk_plan(*shape, "po2"))
    assert torch.isnan(new).any() and torch.isfinite(new).any()
    for other in (old, ref):
        assert torch.equal(torch.isnan(new), torch.isnan(other))
        assert torch.equal(new.view(torch.int32), other.view(torch.int32))


# ------------------------------------------------------------------ the run --
RUN = (2, 64, 7, 56)


@functools.lru_cache(maxsize=None)
def run_case():
    g = torch.Generator().manual_seed(78)
    x = torch.relu(torch.randn(*RUN, generator=g)).to(DEV)
    return x, [kaiming(g).to(DEV) for _ in range(5)]


def one_by_one(x, ws, mode):
    """The chain's own schedule, layer call by layer call: pairs left to right, a leftover single."""
    a, l = x, 0
    while l < len(ws):
        if l + 1 < len(ws):
            a = _lib.qconv2d_pair(a, ws[l], ws[l + 1], 4, mode)
            l += 2
        else:
            a = _lib.qconv2d(a, ws[l], None, 1, 1, 1, 1, 4, mode)
            l += 1
    return a


def test_chain64_pipelined_run_bit_for_bit(monkeypatch):
    x, ws = run_case()
    assert _lib.chain_supported(RUN, len(ws), 4, "po2")
    old, new, _ = both_schedules(monkeypatch, lambda: _lib.qconv2d_chain(x, ws, 4, "po2"))
    assert torch.isfinite(new).all() and float(new.abs().max()) > 0
    assert torch.equal(new, old)
    assert torch.equal(new, one_by_one(x, ws, "po2"))


def test_chain64_pipelined_graph_capture():
    x, ws = run_case()
    eager = _lib.qconv2d_chain(x, ws, 4, "po2")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.qconv2d_chain(x, ws, 4, "po2")
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _lib.qconv2d_chain(x, ws, 4, "po2")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(out, one_by_one(x, ws, "po2"))


# ------------------------------------------------------------ conv_pairw (C = 32) --
WKNOB = "PO2Q_PAIR_W32_PIPE"
# H <= 3: shorter than the pipeline's fill (the prologue split, skipped rows); 6 / 7, 12 / 13: H + 6 steps
# on both sides of the 6-step unroll's break; 23: two row segments at N = 2 (the split-ahead crosses a
# segment's halo).  W = 100 / 108: ragged last strip; 112: the padding group
WSHAPES = [(2, h, w) for h in (1, 2, 3, 6, 7, 12, 13, 23) for w in (100, 108, 112)]
ACTS = {"none": lambda t: t, "relu": torch.relu, "relu6": torch.nn.functional.relu6, "silu": torch.nn.functional.silu}


@functools.lru_cache(maxsize=None)
def wcase(N, H, W):
    g = torch.Generator().manual_seed(9000 + 200 * H + W + N)
    x = torch.randn(N, 32, H, W, generator=g)
    w1, w2 = torch.randn(32, 32, 3, 3, generator=g) * 0.12, torch.randn(32, 32, 3, 3, generator=g) * 0.12
    e = {"post_scale1": torch.rand(32, generator=g) + 0.5, "post_shift1": torch.randn(32, generator=g) * 0.1,
         "post_scale2": torch.rand(32, generator=g) + 0.5, "post_shift2": torch.randn(32, generator=g) * 0.1,
         "bias1": torch.randn(32, generator=g) * 0.1, "bias2": torch.randn(32, generator=g) * 0.1}
    return x, w1, w2, e


def wforms(x, e):
    """(name, keyword arguments, runs the pipelined schedule)."""
    aff = {k: v for k, v in e.items() if k.startswith("post_")}
    return [("plain", {}, True),
            ("general relu/relu6", dict(act1="relu", act2="relu6", **aff), True),
            ("general silu/relu + biases", dict(act1="silu", act2="relu", **e), True),
            ("BasicBlock", dict(act1="relu", act2="relu", residual=x, **aff), False),
            ("general residual", dict(act1="silu", act2="relu", residual=x.flip(3).contiguous(), **e), False)]


def oracle_chain(x, w1, w2, mode, kw):
    """The reference's CPU path for both convs, the epilogues between and after them in torch on the CPU."""
    def epi(t, i):
        if kw.get("bias%d" % i) is not None:
            t = t + kw["bias%d" % i].view(1, -1, 1, 1)
        if kw.get("post_scale%d" % i) is not None:
            t = t * kw["post_scale%d" % i].view(1, -1, 1, 1) + kw["post_shift%d" % i].view(1, -1, 1, 1)
        return t
    h = ACTS[kw.get("act1", "none")](epi(O.cpu_reference_qconv2d(x, w1, None, 1, 1, 1, 1, 4, mode), 1))
    y = epi(O.cpu_reference_qconv2d(h, w2, None, 1, 1, 1, 1, 4, mode), 2)
    if kw.get("residual") is not None:
        y = y + kw["residual"]
    return ACTS[kw.get("act2", "none")](y)


def on_dev(kw):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}


@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("shape", WSHAPES, ids=[str(s) for s in WSHAPES])
def test_pairw_pipelined_bitwise_equal_7wave_kernel(shape, mode, monkeypatch):
    x, w1, w2, e = wcase(*shape)
    xd, w1d, w2d = x.to(DEV), w1.to(DEV), w2.to(DEV)
    for name, kw, _ in wforms(x, e):
        kd = on_dev(kw)
        monkeypatch.setenv("PO2Q_PAIR_W32", "0")
        ref = _lib.qconv2d_pair(xd, w1d, w2d, 4, mode, **kd)
        monkeypatch.setenv("PO2Q_PAIR_W32", "1")
        monkeypatch.setenv(WKNOB, "0")
        old = _lib.qconv2d_pair(xd, w1d, w2d, 4, mode, **kd)
        monkeypatch.delenv(WKNOB)
        y = _lib.qconv2d_pair(xd, w1d, w2d, 4, mode, **kd)
        monkeypatch.delenv("PO2Q_PAIR_W32")
        err = normwise_err(y.cpu().numpy(), oracle_chain(x, w1, w2, mode, kw).numpy())
        print("pairw pipelined", shape, mode, name, "differing elements: vs 7-wave %d, vs old %d; normwise err %.3g"
              % (int((y != ref).sum()), int((y != old).sum()), err))
        assert torch.isfinite(y).all() and float(y.abs().max()) > 0
        assert torch.equal(y, ref), name
        assert torch.equal(y, old), name
        assert err <= CONV_TOL, (name, err)


@pytest.mark.parametrize("shape", [(2, 13, 112), (3, 9, 100)], ids=str)
def test_pairw_pipelined_equals_earlier_schedule(shape, monkeypatch):
    x, w1, w2, e = wcase(*shape)
    xd, w1d, w2d = x.to(DEV), w1.to(DEV), w2.to(DEV)
    for mode in ("po2", "po2+"):
        for name, kw, pipelined in wforms(x, e):
            if not pipelined:
                continue
            kd = on_dev(kw)
            monkeypatch.setenv(WKNOB, "0")
            old = _lib.qconv2d_pair(xd, w1d, w2d, 4, mode, **kd)
            monkeypatch.setenv(WKNOB, "1")
            new = _lib.qconv2d_pair(xd, w1d, w2d, 4, mode, **kd)
            monkeypatch.delenv(WKNOB)
            assert torch.equal(new, old), (mode, name)
            assert torch.equal(_lib.qconv2d_pair(xd, w1d, w2d, 4, mode, **kd), new), (mode, name)  # on by default


@pytest.mark.parametrize("shape", [(2, 7, 100), (2, 13, 112)], ids=str)
def test_pairw_pipelined_nonfinite_inputs(shape, monkeypatch):
    """+-inf and NaN in the first and last image row and in the last valid column: bit for bit the 7-wave
    kernel's output, NaNs and infinities in the same places."""
    N, H, W = shape
    x, w1, w2, e = wcase(*shape)
    x = x.clone()
    x[0, 3, 0, 10] = float("inf")
    x[0, 20, H - 1, W - 1] = float("-inf")
    x[1, 17, H - 1, 0] = float("nan")
    x[1, 31, 0, W - 1] = float("nan")
    x[1, 5, H // 2, W - 1] = float("inf")
    xd, w1d, w2d = x.to(DEV), w1.to(DEV), w2.to(DEV)
    for name, kw, pipelined in wforms(x, e)[:2]:
        kd = on_dev(kw)
        monkeypatch.setenv("PO2Q_PAIR_W32", "0")
        ref = _lib.qconv2d_pair(xd, w1d, w2d, 4, "po2", **kd)
        monkeypatch.delenv("PO2Q_PAIR_W32")
        y = _lib.qconv2d_pair(xd, w1d, w2d, 4, "po2", **kd)
        assert torch.isnan(y).any() and torch.isfinite(y).any()
        assert same_nonfinite(y, ref), name
        assert torch.equal(y.view(torch.int32), ref.view(torch.int32)), name
