"""GPU: the fused attention core (po2q_mhsa_f32, po2_quantization_amd/csrc/po2q_mhsa.hip) through torch.ops.po2q.mhsa,
the C ABI and the MobileViT models, against the reference's formula (models/mobile_vit.py:68-98) in fp64 on the CPU."""
import ctypes
import sys

import pytest
import torch

from po2_quantization_amd import _lib
from po2_quantization_amd.models import mobile_vit
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.utils.quantizers import quantizer_dict
from tests._util import CONV_TOL, GOLDEN, load_npz, normwise_err

sys.path.insert(0, GOLDEN)
from fill import seeded_fill_  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, D = 4, 8
SCALE = D ** -0.5
LOGIT_TOL = CONV_TOL


def make_qkv(S, N, amp=1.0):
    g = torch.Generator().manual_seed(1000 * N + S)
    return torch.randn(S, N, 3 * H * D, generator=g) * amp


def reference(qkv):
    """Attention.forward between to_qkv and to_out, in fp64."""
    S, N, _ = qkv.shape
    q, k, v = (t.view(S, N, H, D).transpose(1, 2) for t in qkv.double().chunk(3, dim=-1))
    attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * SCALE, dim=-1)
    return torch.matmul(attn, v).transpose(1, 2).reshape(S, N, H * D)


# N: a single key, sub-tile, tile edge -1 / 0 / +1 (16 | 17: heads-per-block vs tiles-per-block kernels), a ragged
# multi-tile N with a second query-tile round (70), config 5's sizes (64, 256: four rounds per wave), and more keys
# than one LDS chunk holds with a ragged last chunk (530); amp 4: |score| far above exp's fp32 overflow point
@pytest.mark.parametrize("N,S,amp", [(N, S, 1.0) for N in (1, 4, 15, 16, 17, 64, 70, 256) for S in (1, 3)]
                         + [(530, 1, 1.0), (64, 3, 4.0), (256, 3, 4.0)])
def test_kernel_vs_fp64(N, S, amp):
    qkv = make_qkv(S, N, amp)
    out = _lib.ops().mhsa(qkv.to(DEV), H, SCALE)  # torch.ops.po2q.mhsa
    assert out.shape == (S, N, H * D) and out.dtype == torch.float32
    err = normwise_err(out.cpu().numpy(), reference(qkv).numpy())
    print("mhsa N=%d S=%d amp=%g normwise %.3g" % (N, S, amp, err))
    assert err <= CONV_TOL, err
    if N == 1:
        assert torch.equal(out.cpu(), qkv[..., 2 * H * D:])  # p = 1.0: out is v bit for bit


@pytest.mark.parametrize("N", [5, 40])
def test_direct_head_placement(N):
    qkv = torch.zeros(2, N, 3 * H * D)
    qkv[..., 2 * H * D:] = torch.arange(1.0, H + 1).repeat_interleave(D)  # head h's v is h + 1 everywhere
    out = _lib.mhsa(qkv.to(DEV).view(2, 1, N, -1), H, SCALE).cpu()
    assert out.shape == (2, 1, N, H * D)
    assert torch.equal(out.view(2, N, H * D), qkv[..., 2 * H * D:])


def test_c_abi_on_device_pointers():
    qkv = make_qkv(2, 17)
    x, out = qkv.to(DEV), torch.empty(2, 17, H * D, device=DEV)
    L = _lib.load()
    st = L.po2q_mhsa_f32(x.data_ptr(), out.data_ptr(), 2, 17, H, D, SCALE,
                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, L.po2q_last_error()
    assert normwise_err(out.cpu().numpy(), reference(qkv).numpy()) <= CONV_TOL


@pytest.mark.parametrize("spec", ["mobilevit", "mobilevit@64"])
def test_model_logits_with_native_attention(spec, monkeypatch):
    """Three eval forwards, as test_qat_mode_logits runs them, with the 9 attention layers on the fused kernel."""
    calls = []
    orig = _lib.mhsa
    monkeypatch.setattr(_lib, "mhsa", lambda *a, **k: calls.append(1) or orig(*a, **k))
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
        monkeypatch.setattr(mobile_vit, "NATIVE_ATTENTION", True)
        for i in range(3):
            e = normwise_err(m(x).cpu().numpy(), ref)
            assert e <= LOGIT_TOL, e
            assert len(calls) == 9 * (i + 1)
