"""GPU: the fused LayerNorm + MLP + residual kernels (po2q_ffn_f32, po2_quantization_amd/csrc/po2q_ffn.hip) through
torch.ops.po2q.ffn, the C ABI and the MobileViT models, against the formula of FeedForward and the add around it
(models/mobile_vit.py) in fp64 on the CPU."""
import ctypes
import sys

import pytest
import torch
import torch.nn.functional as F

from po2_quantization_amd import _lib
from po2_quantization_amd.models import mobile_vit
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.utils.quantizers import quantizer_dict
from tests._util import CONV_TOL, GOLDEN, load_npz, normwise_err

sys.path.insert(0, GOLDEN)
from fill import seeded_fill_  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
LOGIT_TOL = CONV_TOL
TILES, SPLIT = 1, 2  # PO2Q_FFN_TOKEN_TILES, PO2Q_FFN_HIDDEN_SPLIT; 0 picks by M (hidden split up to 16384 tokens)
ALL_M = (1, 15, 16, 17, 33, 130)  # tile edge -1 / 0 / +1, a wave's second tile, a second token-tile block


def make_inputs(M, dim, hidden, amp=1.0):
    """x, ln_w, ln_b, w1, b1, w2, b2 on the CPU in fp32; amp scales x and w1."""
    g = torch.Generator().manual_seed(100000 * dim + 100 * hidden + M)
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    return (r(M, dim) * amp, 1 + 0.5 * r(dim), 0.5 * r(dim), r(hidden, dim) * (amp / dim ** 0.5), r(hidden),
            r(dim, hidden) / hidden ** 0.5, r(dim))


def reference(x, ln_w, ln_b, w1, b1, w2, b2, residual=True):
    x, ln_w, ln_b, w1, b1, w2, b2 = (t.double() for t in (x, ln_w, ln_b, w1, b1, w2, b2))
    y = F.linear(F.silu(F.linear(F.layer_norm(x, x.shape[-1:], ln_w, ln_b, EPS), w1, b1)), w2, b2)
    return x + y if residual else y


# (dim, hidden): one partial tile each way (4, 4), (8, 20); exact tiles (16, 16); a ragged dim tile and a ragged hidden
# chunk (24, 36); the two model sizes that are no multiple of 16 tiles wide / need 9 dim tiles (120, 480), (144, 576).
# amp 30: pre-activations pass +-88, where SiLU's exponential overflows.  kernel 0: below and above the auto threshold.
CASES = ([(d, h, M, k, True, 1.0) for d, h in ((4, 4), (8, 20), (120, 480), (144, 576)) for M in ALL_M
          for k in (TILES, SPLIT)]
         + [(d, h, M, k, True, 1.0) for d, h in ((16, 16), (24, 36)) for M in (17, 130) for k in (TILES, SPLIT)]
         + [(8, 20, 17, TILES, False, 1.0), (120, 480, 33, SPLIT, False, 1.0)]
         + [(8, 20, 17, 0, True, 1.0), (8, 20, 16400, 0, True, 1.0)]
         + [(144, 576, 33, TILES, True, 30.0), (144, 576, 33, SPLIT, True, 30.0)])


@pytest.mark.parametrize("dim,hidden,M,kernel,residual,amp", CASES)
def test_kernel_vs_fp64(dim, hidden, M, kernel, residual, amp):
    p = make_inputs(M, dim, hidden, amp)
    x, ln_w, ln_b, w1, b1, w2, b2 = (t.to(DEV) for t in p)
    out = _lib.ops().ffn(x, ln_w, ln_b, EPS, w1, b1, w2, b2, residual, kernel)  # torch.ops.po2q.ffn
    assert out.shape == (M, dim) and out.dtype == torch.float32
    err = normwise_err(out.cpu().numpy(), reference(*p, residual=residual).numpy())
    print("ffn dim=%d hidden=%d M=%d kernel=%d residual=%d amp=%g normwise %.3g" % (dim, hidden, M, kernel, residual,
                                                                                  amp, err))
    assert err <= CONV_TOL, err


@pytest.mark.parametrize("kernel", [TILES, SPLIT])
@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("dim,hidden", [(120, 480), (8, 20)])
def test_exact_placement(dim, hidden, M, kernel):
    """w1 = 0, b1 = 0: the hidden tile is SiLU(0) = 0 and out is x + b2 bit for bit, every element in its place."""
    p = make_inputs(M, dim, hidden)
    x = torch.arange(M, dtype=torch.float32)[:, None] + torch.arange(dim, dtype=torch.float32) / 256
    b2 = torch.arange(1, dim + 1, dtype=torch.float32) / 8
    out = _lib.ffn(x.to(DEV).view(1, M, dim), p[1].to(DEV), p[2].to(DEV), EPS, torch.zeros(hidden, dim, device=DEV),
                   torch.zeros(hidden, device=DEV), p[5].to(DEV), b2.to(DEV), kernel=kernel)
    assert out.shape == (1, M, dim)
    assert torch.equal(out.cpu()[0], x + b2)


def test_c_abi_on_device_pointers():
    M, dim, hidden = 17, 24, 36
    p = make_inputs(M, dim, hidden)
    d = [t.to(DEV) for t in p]
    out = torch.empty(M, dim, device=DEV)
    L = _lib.load()
    st = L.po2q_ffn_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), EPS, d[3].data_ptr(), d[4].data_ptr(),
                        d[5].data_ptr(), d[6].data_ptr(), out.data_ptr(), M, dim, hidden, 1, 0,
                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, L.po2q_last_error()
    assert normwise_err(out.cpu().numpy(), reference(*p).numpy()) <= CONV_TOL


@pytest.mark.parametrize("spec", ["mobilevit", "mobilevit@64"])
def test_model_logits_with_native_ffn(spec, monkeypatch):
    """Three eval forwards with the 9 MLP halves on the fused kernel, then one more with the fused attention too."""
    calls = []
    orig = _lib.ffn
    monkeypatch.setattr(_lib, "ffn", lambda *a, **k: calls.append(1) or orig(*a, **k))
    d = load_npz("models.npz")
    sz = int(spec.partition("@")[2] or 32)
    m = get_model("mobilevit", 10, quantizer_dict["po2+"], 2, (sz, sz))
    seeded_fill_(m, seed=7)
    m = m.to(DEV).eval()
    x = torch.from_numpy(d["x/img64"] if sz == 64 else d["x/cifar8"]).to(DEV)
    ref = d["logits/%s/po2+/2" % spec]
    with torch.no_grad():
        m(x)
        assert calls == []  # off by default
        monkeypatch.setattr(mobile_vit, "NATIVE_FFN", True)
        for i in range(3):
            e = normwise_err(m(x).cpu().numpy(), ref)
            assert e <= LOGIT_TOL, e
            assert len(calls) == 9 * (i + 1)
        monkeypatch.setattr(mobile_vit, "NATIVE_ATTENTION", True)  # the two switches together
        e = normwise_err(m(x).cpu().numpy(), ref)
        assert e <= LOGIT_TOL and len(calls) == 36, (e, len(calls))


def test_trainable_ffn_keeps_its_gradient(monkeypatch):
    """Grad enabled, frozen attention, trainable FeedForward, an input that records no gradient: the MLP half has to
    run the torch ops (the native kernels are forward only), though nothing upstream of it requires grad.

    The frozen attention half is itself eligible for the native kernels, so with the switches on it runs them and the
    output differs from the all-switches-off output by their rounding.  Bit for bit is therefore asserted against the
    forward that differs in NATIVE_FFN alone (same attention path, the MLP half on torch ops in both), and the
    all-switches-off forward has to agree within the parity contract."""
    torch.manual_seed(3)
    tr = mobile_vit.Transformer(24, 1, 4, 8, 48).to(DEV).train()
    attn, ff = tr.layers[0]
    for w in attn.parameters():
        w.requires_grad_(False)
    x = torch.randn(1, 2, 9, 24, device=DEV)
    assert torch.is_grad_enabled() and not x.requires_grad
    off = tr(x)
    monkeypatch.setattr(mobile_vit, "NATIVE_ATTENTION", True)
    monkeypatch.setattr(mobile_vit, "NATIVE_PROJ", True)
    attn_only = tr(x)

    def no_ffn(*a, **k):
        raise AssertionError("the forward-only fused MLP ran under a recorded gradient")

    monkeypatch.setattr(_lib, "ffn", no_ffn)
    monkeypatch.setattr(mobile_vit, "NATIVE_FFN", True)
    y = tr(x)
    assert y.requires_grad
    err = normwise_err(y.detach().cpu().numpy(), off.detach().cpu().numpy())
    print("all switches on vs attention switches on: equal %s; vs all off: normwise %.3g" % (torch.equal(y, attn_only),
                                                                                             err))
    assert torch.equal(y, attn_only)
    assert err <= CONV_TOL, err
    y.sum().backward()
    g = ff.net[1].weight.grad
    assert g is not None and bool(g.abs().max() > 0)
