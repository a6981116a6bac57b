"""GPU parity of the stage-3 conv pair (conv_pair64: 64 -> 64 -> 64, 32 < W <= 64, two chained
QuantizedConv2d.forward calls, reference models/quantized_conv.py:32-38, with the intermediate on
chip) and of the chain entry's large C = 64 geometry that runs a stage-3 run as such pairs.

Direct pair: against the reference's CPU path applied twice (oracle.cpu_reference_qconv2d), bar:
normwise 1e-5 (CONV_TOL, as tests/test_gpu_pair.py), and bit for bit against two single-conv calls on
a conv_rowsk plan.  conv_rowsk's planner starts at segments of 4 rows, so images of fewer than 4 rows
have no such plan: they are held to the oracle bar only (test_rowsk_has_no_plan_below_four_rows).
Run: po2q_qconv2d_chain_f32 bit for bit against the same layers called one by one."""
import functools

import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from po2_quantization_amd import _lib
from tests._util import CONV_TOL, bits_equal, normwise_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HS, WS = (1, 2, 3, 7), (36, 48, 52, 56, 64)
SHAPES = [(2, h, w) for h in HS for w in WS]
# H <= 3: shorter than the pipeline's fill; W = 36 / 52 / 56: a partly filled last group, 36 also an
# empty one (3-group kernel, as 48); W = 64: the full width
BIT_SHAPES = [(2, h, w) for h in (4, 7) for w in WS]


def kaiming(gen, C=64):
    return torch.randn(C, C, 3, 3, generator=gen) * math.sqrt(2.0 / (C * 9))


@functools.lru_cache(maxsize=None)
def case(N, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 * H + W + seed)
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


@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_pair64_vs_oracle(shape, mode):
    x, w1, w2 = case(*shape)
    y = _lib.qconv2d_pair(x.to(DEV), w1.to(DEV), w2.to(DEV), 4, mode).cpu().numpy()
    err = normwise_err(y, reference(*shape, mode))
    print("pair64", shape, mode, "normwise err %.3g" % err)
    assert err <= CONV_TOL, err


@pytest.mark.parametrize("mode", ["po2", "po2+"])
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=[str(s) for s in BIT_SHAPES])
def test_pair64_bit_for_bit_two_rowsk_calls(shape, mode):
    x, w1, w2 = (t.to(DEV) for t in case(*shape))
    plan = rowsk_plan(*shape, mode)
    assert plan is not None
    y = _lib.qconv2d_pair(x, w1, w2, 4, mode)
    y2 = two_singles(x, w1, w2, mode, plan)
    ndiff = int((y != y2).sum())
    print("pair64 vs 2 x conv_rowsk", shape, mode, "differing elements", ndiff)
    assert torch.equal(y, y2)


def test_rowsk_has_no_plan_below_four_rows():
    for h in (1, 2, 3):
        assert rowsk_plan(2, h, 56, "po2") is None
    assert rowsk_plan(2, 4, 56, "po2") is not None


@pytest.mark.parametrize("mode", ["po2", "po2+"])
def test_pair64_row_segments(mode, monkeypatch):
    """Two row segments: the intermediate rows at the cut are recomputed by both blocks, not zeroed."""
    shape = (2, 9, 56)
    x, w1, w2 = case(*shape)
    xd, w1d, w2d = x.to(DEV), w1.to(DEV), w2.to(DEV)
    one = _lib.qconv2d_pair(xd, w1d, w2d, 4, mode)
    monkeypatch.setenv("PO2Q_PAIR64_NSEG", "2")
    y = _lib.qconv2d_pair(xd, w1d, w2d, 4, mode)
    err = normwise_err(y.cpu().numpy(), reference(*shape, mode))
    print("pair64 2 segments", mode, "normwise err %.3g" % err)
    assert err <= CONV_TOL, err
    assert torch.equal(y, one)
    assert torch.equal(y, two_singles(xd, w1d, w2d, mode, rowsk_plan(*shape, mode)))


def test_pair64_bias():
    shape = (2, 7, 52)
    x, w1, w2 = (t.to(DEV) for t in case(*shape))
    g = torch.Generator().manual_seed(3)
    b1, b2 = (torch.randn(64, generator=g) * 0.1).to(DEV), (torch.randn(64, generator=g) * 0.1).to(DEV)
    y = _lib.qconv2d_pair(x, w1, w2, 4, "po2", bias1=b1, bias2=b2)
    plan = rowsk_plan(*shape, "po2")
    h = _lib.qconv2d(x, w1, b1, 1, 1, 1, 1, 4, "po2", plan=plan)
    assert torch.equal(y, _lib.qconv2d(h, w2, b2, 1, 1, 1, 1, 4, "po2", plan=plan))


def test_pair64_refuses_epilogue_forms():
    x, w1, w2 = (t.to(DEV) for t in case(2, 7, 56))
    with pytest.raises(_lib.Po2qError, match="plain form"):
        _lib.qconv2d_pair(x, w1, w2, 4, "po2", act1="relu")
    with pytest.raises(_lib.Po2qError, match="plain form"):
        _lib.qconv2d_pair(x, w1, w2, 4, "po2", residual=x)


def test_pair64_nonfinite_inputs():
    """One +inf and one NaN in x propagate as they do through two single calls."""
    shape = (2, 7, 56)
    x, w1, w2 = case(*shape)
    x = x.clone()
    x[0, 3, 2, 40] = float("inf")
    x[1, 17, 6, 0] = float("nan")
    xd, w1d, w2d = x.to(DEV), w1.to(DEV), w2.to(DEV)
    y = _lib.qconv2d_pair(xd, w1d, w2d, 4, "po2").cpu().numpy()
    y2 = two_singles(xd, w1d, w2d, "po2", rowsk_plan(*shape, "po2")).cpu().numpy()
    assert np.isnan(y).any() and np.isfinite(y).any()
    assert np.array_equal(np.isnan(y), np.isnan(y2))
    assert bits_equal(y, y2).all()


# ------------------------------------------------------------------ the run --
RUN = (2, 64, 6, 56)


@functools.lru_cache(maxsize=None)
def run_case(n):
    g = torch.Generator().manual_seed(77)
    x = torch.relu(torch.randn(*RUN, generator=g)).to(DEV)
    return x, [kaiming(g).to(DEV) for _ in range(n)]


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


@pytest.mark.parametrize("n", [2, 3, 17])
def test_chain64_plain_run_bit_for_bit(n):
    x, ws = run_case(17)
    ws = ws[:n]
    assert _lib.chain_supported(RUN, n, 4, "po2")
    y = _lib.qconv2d_chain(x, ws, 4, "po2")
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    assert torch.equal(y, one_by_one(x, ws, "po2"))
    if n == 3:  # and every layer as a single conv: the pair kernel adds nothing of its own
        a = x
        plan = rowsk_plan(RUN[0], RUN[2], RUN[3], "po2")
        for w in ws[:2]:
            a = _lib.qconv2d(a, w, None, 1, 1, 1, 1, 4, "po2", plan=plan)
        assert torch.equal(y, _lib.qconv2d(a, ws[2], None, 1, 1, 1, 1, 4, "po2"))


def test_chain64_basic_blocks_vs_fused_calls():
    """Two BasicBlocks (biases, BN affine, ReLU, identity shortcut): every layer takes the fused
    single-conv path, bit for bit the per-layer qconv2d_fused calls."""
    x, ws = run_case(17)
    ws = ws[:4]
    g = torch.Generator().manual_seed(5)
    bs = [(torch.randn(64, generator=g) * 0.1).to(DEV) for _ in ws]
    ps = [(torch.rand(64, generator=g) + 0.5).to(DEV) for _ in ws]
    pb = [(torch.randn(64, generator=g) * 0.1).to(DEV) for _ in ws]
    res = [None, 0, None, 2]
    y = _lib.qconv2d_chain(x, ws, 4, "po2+", biases=bs, post_scales=ps, post_shifts=pb, acts=["relu"] * 4,
                           res_from=res)
    acts, a = [x], x
    for l, w in enumerate(ws):
        r = None if res[l] is None else acts[res[l]]
        a = _lib.qconv2d_fused(a, w, bs[l], 1, 1, 1, 1, 4, "po2+", post_scale=ps[l], post_shift=pb[l], residual=r,
                               act="relu")
        acts.append(a)
    assert torch.equal(y, a)


def test_chain64_mixed_forms():
    """A plain pair, then a layer with an epilogue whose input is a residual source, then a plain
    leftover: pair + single + single, the buffers rotating around the live residual."""
    x, ws = run_case(17)
    ws = ws[:4]
    y = _lib.qconv2d_chain(x, ws, 4, "po2", acts=["none", "none", "relu", "none"], res_from=[None, None, 2, None])
    a = _lib.qconv2d_pair(x, ws[0], ws[1], 4, "po2")
    b = _lib.qconv2d_fused(a, ws[2], None, 1, 1, 1, 1, 4, "po2", residual=a, act="relu")
    assert torch.equal(y, _lib.qconv2d(b, ws[3], None, 1, 1, 1, 1, 4, "po2"))


def test_chain64_graph_capture():
    x, ws = run_case(17)
    ws = ws[:5]
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
