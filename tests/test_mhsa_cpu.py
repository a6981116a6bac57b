"""No device: the attention switch's default, the ptq option, the op's Meta kernel, po2q_mhsa_f32's host-side
argument checks, and the torch path of Attention.forward with the switch on (CPU tensors, recorded gradients)."""
import pytest
import torch

from po2_quantization_amd import _lib, ptq
from po2_quantization_amd.models import mobile_vit


def test_switch_default_ptq_option_and_meta_kernel():
    assert mobile_vit.NATIVE_ATTENTION is False  # opt-in
    a = ptq.arg_parser().parse_args(["mobilevit", "cifar10", "--data_file", "x", "--native-attention"])
    assert a.native_attention
    for shape in ((6, 17, 96), (2, 3, 17, 96)):
        y = _lib.ops().mhsa(torch.empty(shape, device="meta"), 4, 0.5)
        assert y.device.type == "meta" and y.dtype == torch.float32 and tuple(y.shape) == shape[:-1] + (32,)


@pytest.mark.parametrize("over,msg", [({"heads": 3}, b"heads"), ({"dim_head": 16}, b"dim_head"), ({"N": 0}, b"positive"),
                                      ({"S": 0}, b"positive"), ({"qkv": None}, b"null"), ({"out": None}, b"null")])
def test_c_abi_rejects_before_launch(over, msg):
    L = _lib.load()
    buf = torch.zeros(64)  # never dereferenced: every error returns before any launch
    a = dict(qkv=buf.data_ptr(), out=buf.data_ptr(), S=2, N=5, heads=4, dim_head=8)
    a.update(over)
    assert L.po2q_mhsa_f32(a["qkv"], a["out"], a["S"], a["N"], a["heads"], a["dim_head"], 0.35, None) == 1
    assert msg in L.po2q_last_error()


def test_torch_path_is_kept_on_cpu_and_under_grad(monkeypatch):
    torch.manual_seed(5)
    attn = mobile_vit.Attention(24, 4, 8).eval()
    x = torch.randn(2, 4, 9, 24)
    with torch.no_grad():
        want = attn(x)
    monkeypatch.setattr(mobile_vit, "NATIVE_ATTENTION", True)
    monkeypatch.setattr(_lib, "mhsa", lambda *a, **k: pytest.fail("the torch path reached the native kernel"))
    with torch.no_grad():
        assert torch.equal(attn(x), want)
    got = attn(x)  # a gradient is being recorded
    assert got.requires_grad and torch.equal(got.detach(), want)
