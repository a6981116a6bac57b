"""GPU: the fused LayerNorm + Linear + residual kernels (po2q_ln_linear_f32, po2_quantization_amd/csrc/po2q_lnlin.hip)
through torch.ops.po2q.ln_linear, the C ABI and the MobileViT models, against the formula in fp64 on the CPU."""
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
RESIDENT, SPLIT = 1, 2  # PO2Q_LNLIN_RESIDENT, PO2Q_LNLIN_OUT_SPLIT; 0 picks by M (out split up to SPLIT_MAX_M tokens)
BOTH = (RESIDENT, SPLIT)
SPLIT_MAX_M = 8192      # kSplitMaxM in po2q_lnlin.hip
GRID_CAP = 512          # kGridCap: resident blocks in x, 4 token tiles each
MAX_IN = 640            # PO2Q_LNLIN_MAX_IN
ALL_M = (1, 15, 16, 17, 33, 130)  # tile edge -1 / 0 / +1, a second tile in a wave's stride, a second block
QKV, OUT, ALL, NONE = "qkv", "out", "all", "none"  # LN only / bias + residual / all three / none of the three
SMALL = ((4, 4), (8, 20), (16, 16), (24, 36))  # partial tiles both ways, exact tiles, a ragged tile each way


def make_inputs(M, in_dim, out_dim, opts, shift=0.0):
    """x, ln_w, ln_b, w, bias, residual on the CPU in fp32 (None for what opts leaves out); x * shift + shift."""
    g = torch.Generator().manual_seed(100000 * in_dim + 100 * out_dim + M)
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    x, ln_w, ln_b, w = r(M, in_dim), 1 + 0.5 * r(in_dim), 0.5 * r(in_dim), r(out_dim, in_dim) / in_dim ** 0.5
    bias, residual = r(out_dim), r(M, out_dim)
    if shift:
        x = x * shift + shift
    ln = opts in (QKV, ALL)
    br = opts in (OUT, ALL)
    return (x, ln_w if ln else None, ln_b if ln else None, w, bias if br else None, residual if br else None)


def reference(x, ln_w, ln_b, w, bias, residual):
    d = lambda t: None if t is None else t.double()  # noqa: E731
    x = d(x)
    if ln_w is not None:
        x = F.layer_norm(x, x.shape[-1:], d(ln_w), d(ln_b), EPS)
    y = F.linear(x, d(w), d(bias))
    return y if residual is None else d(residual) + y


def run(p, kernel):
    x, ln_w, ln_b, w, bias, residual = (None if t is None else t.to(DEV) for t in p)
    return _lib.ops().ln_linear(x, ln_w, ln_b, EPS, w, bias, residual, kernel)  # torch.ops.po2q.ln_linear


# (in_dim, out_dim, M, kernel, options, shift).  (256, 80): two out chunks in the resident kernel's 64 KB of LDS;
# kernel 0 on both sides of the auto threshold; M = 64 * GRID_CAP + 17: a resident wave's second grid-stride trip;
# shift 1e3: x * 1e3 + 1e3, a large mean against the spread (torch's own fp32 sequence on the CPU is at 3.2e-7 there).
CASES = ([(i, o, M, k, QKV, 0.0) for i, o in ((120, 96), (144, 96)) for M in ALL_M for k in BOTH]
         + [(i, o, M, k, OUT, 0.0) for i, o in ((32, 120), (32, 144)) for M in ALL_M for k in BOTH]
         + [(i, o, M, k, ALL, 0.0) for i, o in SMALL for M in ALL_M for k in BOTH]
         + [(i, o, M, k, NONE, 0.0) for i, o in SMALL for M in (17, 130) for k in BOTH]
         + [(256, 80, M, k, ALL, 0.0) for M in (17, 130) for k in BOTH]
         + [(MAX_IN, 16, 17, k, ALL, 0.0) for k in BOTH]
         + [(8, 20, 17, 0, ALL, 0.0), (8, 20, SPLIT_MAX_M + 16, 0, ALL, 0.0)]
         + [(8, 20, 64 * GRID_CAP + 17, RESIDENT, ALL, 0.0)]
         + [(144, 96, 33, k, QKV, 1e3) for k in BOTH])


@pytest.mark.parametrize("in_dim,out_dim,M,kernel,opts,shift", CASES)
def test_kernel_vs_fp64(in_dim, out_dim, M, kernel, opts, shift):
    p = make_inputs(M, in_dim, out_dim, opts, shift)
    out = run(p, kernel)
    assert out.shape == (M, out_dim) and out.dtype == torch.float32
    err = normwise_err(out.cpu().numpy(), reference(*p).numpy())
    print("ln_linear in=%d out=%d M=%d kernel=%d opts=%s shift=%g normwise %.3g" % (in_dim, out_dim, M, kernel, opts,
                                                                                  shift, err))
    assert err <= CONV_TOL, err


@pytest.mark.parametrize("kernel", BOTH)
@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("in_dim,out_dim", [(32, 120), (8, 20)])
def test_exact_placement(in_dim, out_dim, M, kernel):
    """w = 0: out is residual + bias; w = eye: out is x (products by 1.0 and 0).  Bit for bit, every element."""
    x = torch.arange(M, dtype=torch.float32)[:, None] + torch.arange(in_dim, dtype=torch.float32) / 256
    res = torch.arange(M, dtype=torch.float32)[:, None] - torch.arange(out_dim, dtype=torch.float32) / 128
    bias = torch.arange(1, out_dim + 1, dtype=torch.float32) / 8
    out = _lib.ln_linear(x.to(DEV).view(1, M, in_dim), torch.zeros(out_dim, in_dim, device=DEV), bias=bias.to(DEV),
                         residual=res.to(DEV).view(1, M, out_dim), kernel=kernel)
    assert out.shape == (1, M, out_dim)
    assert torch.equal(out.cpu()[0], res + bias)
    out = _lib.ln_linear(x.to(DEV), torch.eye(in_dim, device=DEV), kernel=kernel)
    assert torch.equal(out.cpu(), x)


def test_c_abi_on_device_pointers():
    M, in_dim, out_dim = 17, 24, 36
    L = _lib.load()
    for opts in (QKV, OUT):  # NULL for the absent operands
        p = make_inputs(M, in_dim, out_dim, opts)
        ptr = [None if t is None else t.to(DEV) for t in p]
        out = torch.empty(M, out_dim, device=DEV)
        a = [None if t is None else t.data_ptr() for t in ptr]
        st = L.po2q_ln_linear_f32(a[0], a[1], a[2], EPS, a[3], a[4], a[5], out.data_ptr(), M, in_dim, out_dim, 0,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, L.po2q_last_error()
        assert normwise_err(out.cpu().numpy(), reference(*p).numpy()) <= CONV_TOL


@pytest.mark.parametrize("spec", ["mobilevit", "mobilevit@64"])
def test_model_logits_with_native_proj(spec, monkeypatch):
    """Eval forwards with both projections of the 9 attention halves on the fused kernel (18 calls per forward), then
    one more with the fused attention core and the fused MLP too."""
    calls = []
    orig = _lib.ln_linear
    monkeypatch.setattr(_lib, "ln_linear", lambda *a, **k: calls.append(1) or orig(*a, **k))
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
        monkeypatch.setattr(mobile_vit, "NATIVE_PROJ", True)
        for i in range(2):
            e = normwise_err(m(x).cpu().numpy(), ref)
            assert e <= LOGIT_TOL, e
            assert len(calls) == 18 * (i + 1)
        monkeypatch.setattr(mobile_vit, "NATIVE_ATTENTION", True)  # the three switches together
        monkeypatch.setattr(mobile_vit, "NATIVE_FFN", True)
        e = normwise_err(m(x).cpu().numpy(), ref)
        assert e <= LOGIT_TOL and len(calls) == 54, (e, len(calls))
