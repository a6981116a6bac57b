"""GPU parity of the native lin / lin+ conv modes (PO2Q_MODE_LIN / PO2Q_MODE_LIN_PLUS).

Reference weight: O.quantize_lin (pinned bit-exact to the reference's golden vectors); reference
conv: O.conv2d in fp64; bar: CONV_TOL normwise (tests/_util.py).  The impulse tests read the packed
weight back through the conv and ask bit equality with the lin quantizer's own output."""
import ctypes
import sys
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from po2_quantization_amd import _lib
from po2_quantization_amd.models import quantized_conv as qc
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.models.quantized_conv import QuantizedConv2d, fold_bn
from po2_quantization_amd.utils.quantizers import quantizer_dict
from tests._util import CONV_TOL, GOLDEN, load_npz, normwise_err

sys.path.insert(0, GOLDEN)
from fill import seeded_fill_  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERS = 10
LOGIT_TOL = CONV_TOL
MODES = ["lin", "lin+"]

# N, C, H, W, K, R, S, stride, pad, dil, groups (from tests/test_gpu_conv.py SHAPES)
SHAPES = [
    (2, 16, 40, 36, 16, 3, 3, 1, 1, 1, 1),
    (2, 32, 20, 20, 32, 3, 3, 1, 1, 1, 1),
    (1, 64, 14, 14, 64, 3, 3, 1, 1, 1, 1),
    (2, 16, 33, 31, 32, 3, 3, 2, 1, 1, 1),
    (2, 32, 16, 16, 64, 1, 1, 2, 0, 1, 1),
    (2, 160, 4, 4, 960, 1, 1, 1, 0, 1, 1),
    (2, 48, 9, 9, 24, 3, 3, 1, 1, 1, 1),
    (2, 144, 8, 8, 144, 3, 3, 2, 1, 1, 144),
    (1, 20, 13, 11, 36, 3, 3, 1, 2, 2, 2),
    (2, 16, 1, 36, 16, 3, 3, 1, 1, 1, 1),
    (1, 64, 3, 8, 64, 3, 3, 1, 1, 1, 1),
    (1, 16, 9, 220, 16, 3, 3, 1, 1, 1, 1),
]


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0xFFFF


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None


def nplans(shape, bits, mode, iters=ITERS, precision="auto"):
    N, C, H, W, K, R, S, st, pad, dil, groups = shape
    return len(_lib.plans(N, C, H, W, K, R, S, st, pad, dil, groups, bits, mode, iters, precision))


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_every_plan_vs_oracle(shape, mode, bits):
    N, C, H, W, K, R, S, st, pad, dil, groups = shape
    g = torch.Generator().manual_seed(seed_of(shape, mode, bits))
    x = torch.randn(N, C, H, W, generator=g).numpy()
    w = (torch.randn(K, C // groups, R, S, generator=g) * 0.2).numpy()
    b = torch.randn(K, generator=g).numpy() if K % 3 == 0 else None
    qw = O.quantize_lin(w, bits, mode == "lin+", ITERS)
    ref = O.conv2d(x, qw, b, st, pad, dil, groups)
    assert np.isfinite(ref).all()
    xt, wt, bt = dev(x), dev(w), dev(b)
    n = nplans(shape, bits, mode)
    assert n >= 1
    for i in range(n):
        y = _lib.qconv2d(xt, wt, bt, st, pad, dil, groups, bits, mode, ITERS, "auto", plan=i).cpu().numpy()
        err = normwise_err(y, ref)
        assert err <= CONV_TOL, (i, err)
    y = _lib.qconv2d(xt, wt, bt, st, pad, dil, groups, bits, mode, ITERS, "auto").cpu().numpy()
    assert normwise_err(y, ref) <= CONV_TOL


# C, K, R, groups: the packed weight read back through the conv, in every layout
IMPULSE = [(16, 16, 3, 1), (32, 32, 3, 1), (64, 64, 3, 1), (24, 40, 3, 1), (96, 24, 1, 1), (32, 32, 3, 32)]


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("bits", [4, 9])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", IMPULSE, ids=[str(c) for c in IMPULSE])
def test_impulse_reads_back_the_quantizer_output(case, mode, bits, precision):
    C, K, R, groups = case
    g = torch.Generator().manual_seed(seed_of(case, mode, bits))
    w = (torch.randn(K, C // groups, R, R, generator=g) * 0.2).to(DEV)
    q = _lib.quantize_lin(w, bits, mode == "lin+").cpu().numpy()
    assert np.isfinite(q).all()
    pad = 1 if R == 3 else 0
    if groups == 1:
        x = torch.zeros(C, C, 8, 8)
        for i in range(C):
            x[i, i, 4, 4] = 1.0
    else:  # depthwise: one image with an impulse in every channel
        x = torch.zeros(1, C, 8, 8)
        x[0, :, 4, 4] = 1.0
    x = x.to(DEV)
    shape = (x.shape[0], C, 8, 8, K, R, R, 1, pad, 1, groups)
    n = nplans(shape, bits, mode, precision=precision)
    assert n >= 1
    if groups > 1:
        want = q[:, 0, ::-1, ::-1][None]                     # y[0, k, 3 + a, 3 + b] = Q[k, 0, 2 - a, 2 - b]
    elif R == 3:
        want = q.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]     # y[i, k, p, q] = Q[k, i, 5 - p, 5 - q]
    else:
        want = q.transpose(1, 0, 2, 3)                       # y[i, k, 4, 4] = Q[k, i, 0, 0]
    for i in range(n):
        y = _lib.qconv2d(x, w, None, 1, pad, 1, groups, bits, mode, ITERS, precision, plan=i).cpu().numpy()
        got = y[:, :, 3:6, 3:6] if R == 3 else y[:, :, 4:5, 4:5]
        assert np.array_equal(got, want), (i, np.abs(got - want).max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("over", [dict(bits=10), dict(iters=0), dict(groups=2)], ids=["bits10", "iters0", "groups2"])
def test_precision_routing(over, mode):
    bits, iters, groups = over.get("bits", 4), over.get("iters", ITERS), over.get("groups", 1)
    N, C, H, W, K = 2, 16, 10, 12, 16
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, C, H, W, generator=g).numpy()
    w = (torch.randn(K, C // groups, 3, 3, generator=g) * 0.2).numpy()
    ref = O.conv2d(x, O.quantize_lin(w, bits, mode == "lin+", iters), None, 1, 1, 1, groups)
    y = _lib.qconv2d(dev(x), dev(w), None, 1, 1, 1, groups, bits, mode, iters, "auto").cpu().numpy()
    assert normwise_err(y, ref) <= CONV_TOL, normwise_err(y, ref)
    with pytest.raises(RuntimeError, match="bf16x3"):
        _lib.qconv2d(dev(x), dev(w), None, 1, 1, 1, groups, bits, mode, iters, "bf16x3")


# N, C, H, W, K, R, stride, pad, groups
FUSED_SHAPES = [(2, 16, 20, 32, 16, 3, 1, 1, 1), (1, 64, 9, 40, 64, 3, 1, 1, 1), (2, 96, 5, 5, 24, 1, 1, 0, 1),
                (2, 32, 8, 8, 32, 3, 1, 1, 32)]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("act", ["relu", "relu6", "silu"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=[str(s) for s in FUSED_SHAPES])
def test_fused_epilogue_vs_fp64(shape, act, with_res):
    """po2q_qconv2d_fused_f32 in mode lin == act(bn_eval(conv(x, Q(w))) + residual), the formula in fp64."""
    N, C, H, W, K, R, st, pad, groups = shape
    g = torch.Generator().manual_seed(seed_of(shape, act, with_res))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C // groups, R, R, generator=g) * 0.2
    bn = torch.nn.BatchNorm2d(K).eval()
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * torch.randn(K, generator=g))
        bn.bias.copy_(0.1 * torch.randn(K, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(K, generator=g))
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
    y0 = O.conv2d(x.numpy(), O.quantize_lin(w.numpy(), 4, False, ITERS), None, st, pad, 1, groups)
    v = lambda t: t.detach().double().numpy().reshape(1, -1, 1, 1)  # noqa: E731
    y0 = (y0 - v(bn.running_mean)) / np.sqrt(v(bn.running_var) + bn.eps) * v(bn.weight) + v(bn.bias)
    res = torch.randn(y0.shape, generator=g) if with_res else None
    if with_res:
        y0 = y0 + res.double().numpy()
    acts = {"relu": lambda t: np.maximum(t, 0.0), "relu6": lambda t: np.clip(t, 0.0, 6.0),
            "silu": lambda t: t / (1.0 + np.exp(-t))}
    ref = acts[act](y0)
    bn = bn.to(DEV)
    with torch.no_grad():
        ps, pb = fold_bn(bn)
        y = _lib.qconv2d_fused(x.to(DEV), w.to(DEV), None, st, pad, 1, groups, 4, "lin", ITERS, post_scale=ps,
                               post_shift=pb, residual=res.to(DEV) if with_res else None, act=act)
    err = normwise_err(y.cpu().numpy(), ref)
    assert err <= CONV_TOL, err


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(2, 16, 12, 16, 16, 3, 1, 1), (2, 96, 5, 5, 24, 1, 0, 1), (2, 32, 8, 8, 32, 3, 1, 32)],
                         ids=["3x3", "1x1", "depthwise"])
def test_pack_then_packed_equals_qconv2d(shape, mode):
    """The two-enqueue form (po2q_qconv2d_pack_f32 / _packed_f32) and the batched pack
    (qconv2d_pack_batch / qconv2d_packed) on one stream: bit for bit qconv2d's result."""
    N, C, H, W, K, R, pad, groups = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H, W, generator=g).to(DEV)
    w = (torch.randn(K, C // groups, R, R, generator=g) * 0.2).to(DEV)
    ref = _lib.qconv2d(x, w, None, 1, pad, 1, groups, 4, mode, ITERS)
    sc = _lib.SplitConv(x.shape, w, 1, pad, 1, groups, 4, mode, ITERS)
    sc.pack()
    assert torch.equal(sc.conv(x), ref)
    ws = _lib.pack_batch([(w, x.shape, 1, pad, 1, groups)], 4, mode, ITERS)
    assert ws[0].numel() > 0
    assert torch.equal(_lib.qconv2d_packed(x, w, ws[0], None, 1, pad, 1, groups, 4, mode, ITERS), ref)


def test_mixed_pack_batch_equals_per_layer_calls():
    """po2q_qconv2d_plan_pack_batch on plans of different modes -- one po2 3x3, one lin 3x3, one lin+ 1x1,
    one lin depthwise -- then each conv from its pack: bit for bit the per-layer calls."""
    L = _lib.load()
    g = torch.Generator().manual_seed(9)
    # (x shape, K, R, pad, groups, mode, fsr)
    layers = [((2, 16, 12, 16), 16, 3, 1, 1, "po2", 1), ((2, 32, 8, 8), 32, 3, 1, 1, "lin", ITERS),
              ((2, 96, 5, 5), 24, 1, 0, 1, "lin+", ITERS), ((2, 32, 8, 8), 32, 3, 1, 32, "lin", ITERS)]
    xs, wts, hs, wss, refs = [], [], [], [], []
    try:
        for (N, C, H, W), K, R, pad, groups, mode, fsr in layers:
            x = torch.randn(N, C, H, W, generator=g).to(DEV)
            w = (torch.randn(K, C // groups, R, R, generator=g) * 0.2).to(DEV)
            refs.append(_lib.qconv2d(x, w, None, 1, pad, 1, groups, 4, mode, fsr, plan=0))
            h = ctypes.c_void_p()
            _lib._check(L.po2q_qconv2d_plan_create(ctypes.byref(h), 0, N, C, H, W, K, R, R, 1, 1, pad, pad, 1, 1,
                                                    groups, 4, fsr, _lib.MODES[mode], 0))
            assert L.po2q_qconv2d_plan_packs_weight(h) == 1
            xs.append(x)
            wts.append(w)
            hs.append(h)
            wss.append(torch.zeros(L.po2q_qconv2d_plan_workspace_bytes(h), dtype=torch.uint8, device=DEV))
        n = len(hs)
        pa = (ctypes.c_void_p * n)(*[h.value for h in hs])
        wa = (ctypes.c_void_p * n)(*[w.data_ptr() for w in wts])
        sa = (ctypes.c_void_p * n)(*[t.data_ptr() for t in wss])
        ba = (ctypes.c_size_t * n)(*[t.numel() for t in wss])
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib._check(L.po2q_qconv2d_plan_pack_batch(n, pa, wa, sa, ba, stream))
        for i in range(n):
            y = torch.empty_like(refs[i])
            _lib._check(L.po2q_qconv2d_plan_run_packed(hs[i], xs[i].data_ptr(), wts[i].data_ptr(), None, y.data_ptr(),
                                                       None, None, None, 0, wss[i].data_ptr(), wss[i].numel(), stream))
            assert torch.equal(y, refs[i]), i
    finally:
        torch.cuda.synchronize()
        for h in hs:
            L.po2q_qconv2d_plan_destroy(h)


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("mode", MODES)
def test_constant_channel_gives_nan_everywhere(mode, precision):
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 16, 10, 12, generator=g)
    w = torch.randn(16, 16, 3, 3, generator=g) * 0.2
    w[:, 3] = 0.5  # a constant input channel: step 0, Q(w) NaN in that channel
    ref = O.conv2d(x.numpy(), O.quantize_lin(w.numpy(), 4, mode == "lin+", ITERS), None, 1, 1, 1, 1)
    assert np.isnan(ref).all()
    n = nplans((2, 16, 10, 12, 16, 3, 3, 1, 1, 1, 1), 4, mode, precision=precision)
    for i in range(n):
        y = _lib.qconv2d(x.to(DEV), w.to(DEV), None, 1, 1, 1, 1, 4, mode, ITERS, precision, plan=i)
        assert torch.isnan(y).all().item(), i


@pytest.mark.parametrize("mode", MODES)
def test_module_routes_lin_through_the_native_mode(mode, monkeypatch):
    seen = []
    orig, orig_fused = _lib.qconv2d, _lib.qconv2d_fused
    monkeypatch.setattr(_lib, "qconv2d", lambda *a, **k: seen.append(a[8]) or orig(*a, **k))
    monkeypatch.setattr(_lib, "qconv2d_fused", lambda *a, **k: seen.append(a[8]) or orig_fused(*a, **k))
    torch.manual_seed(17)
    mod = QuantizedConv2d(16, 16, 3, quantize_fn=quantizer_dict[mode]).eval()
    x = torch.randn(2, 16, 12, 12)
    with torch.no_grad():
        ref = mod(x).numpy()
        mod = mod.to(DEV)
        y = mod(x.to(DEV)).cpu().numpy()
        yf = mod.fused(x.to(DEV)).cpu().numpy()
    assert seen == [mode, mode], seen
    assert normwise_err(y, ref) <= CONV_TOL and normwise_err(yf, ref) <= CONV_TOL
    seen.clear()
    monkeypatch.setattr(qc, "NATIVE_LIN", False)
    with torch.no_grad():
        y = mod(x.to(DEV)).cpu().numpy()
        yf = mod.fused(x.to(DEV)).cpu().numpy()
    assert seen == ["none", "none"], seen
    assert normwise_err(y, ref) <= CONV_TOL and normwise_err(yf, ref) <= CONV_TOL


@pytest.mark.parametrize("cin,cout,stride,groups", [(16, 16, 1, 1), (16, 32, 2, 1), (32, 32, 1, 32)],
                         ids=["3x3s1", "3x3s2", "depthwise"])
def test_backward_matches_the_cpu_module(cin, cout, stride, groups):
    torch.manual_seed(19)
    cpu = QuantizedConv2d(cin, cout, 3, stride=stride, groups=groups, quantize_fn=quantizer_dict["lin"])
    gpu = QuantizedConv2d(cin, cout, 3, stride=stride, groups=groups, quantize_fn=quantizer_dict["lin"])
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.to(DEV)
    x = torch.randn(2, cin, 12, 12)
    xc = x.clone().requires_grad_(True)
    xg = x.to(DEV).requires_grad_(True)
    yc = cpu(xc)
    gy = torch.randn(yc.shape)
    yc.backward(gy)
    before = qc.ATEN_BACKWARD_CALLS
    yg = gpu(xg)
    yg.backward(gy.to(DEV))
    assert qc.ATEN_BACKWARD_CALLS == before
    assert normwise_err(yg.detach().cpu().numpy(), yc.detach().numpy()) <= CONV_TOL
    assert normwise_err(xg.grad.cpu().numpy(), xc.grad.numpy()) <= CONV_TOL
    assert normwise_err(gpu.weight.grad.cpu().numpy(), cpu.weight.grad.numpy()) <= CONV_TOL


def build_model(mt, q, bits):
    m = get_model(mt, 10, quantizer_dict[q], bits, (32, 32))
    seeded_fill_(m, seed=7)
    return m.to(DEV).eval()


def count_calls(monkeypatch):
    calls = {}
    for name in ("qconv2d_packed", "qconv2d_pair", "qconv2d_s2ds", "qconv2d_chain", "qconv2d_ir"):
        calls[name] = 0

        def counted(*a, _n=name, _f=getattr(_lib, name), **k):
            calls[_n] += 1
            return _f(*a, **k)

        monkeypatch.setattr(_lib, name, counted)
    return calls


@pytest.mark.parametrize("mt,q,bits", [("resnet20", "lin", 4), ("mobilenet", "lin+", 4)])
def test_model_logits_three_eval_forwards(mt, q, bits, monkeypatch):
    """Recording forward, then two from the batched packs; the reference's logits
    (tests/golden/gen_golden_lin.py) every time; never a multi-layer kernel."""
    calls = count_calls(monkeypatch)
    d = load_npz("models_lin.npz")
    m = build_model(mt, q, bits)
    x = torch.from_numpy(d["x/cifar8"]).to(DEV)
    ref = d["logits/%s/%s/%d" % (mt, q, bits)]
    assert np.isfinite(ref).all()
    with torch.no_grad():
        y1 = m(x).cpu().numpy()
        assert calls["qconv2d_packed"] == 0  # the recording forward: per-layer calls
        y2 = m(x).cpu().numpy()
        n2 = calls["qconv2d_packed"]
        y3 = m(x).cpu().numpy()
    for y in (y1, y2, y3):
        assert normwise_err(y, ref) <= LOGIT_TOL, normwise_err(y, ref)
    assert n2 > 0 and calls["qconv2d_packed"] == 2 * n2, calls
    for name in ("qconv2d_pair", "qconv2d_s2ds", "qconv2d_chain", "qconv2d_ir"):
        assert calls[name] == 0, calls


def test_graph_capture_replays_the_eager_logits():
    d = load_npz("models_lin.npz")
    m = build_model("resnet20", "lin", 4)
    x = torch.from_numpy(d["x/cifar8"]).to(DEV)
    with torch.no_grad():
        m(x)
        eager = m(x).clone()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = m(x)
        gr.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert normwise_err(out.cpu().numpy(), d["logits/resnet20/lin/4"]) <= LOGIT_TOL
