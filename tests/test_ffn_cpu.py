"""No device: the MLP switch's default, the ptq option, the op's Meta kernel, po2q_ffn_f32's host-side argument
checks, and the torch path of Transformer.forward with the switch on (CPU tensors, recorded gradients, dropout)."""
import pytest
import torch

from po2_quantization_amd import _lib, ptq
from po2_quantization_amd.models import mobile_vit

PTRS = ("x", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "out")


def test_switch_default_ptq_option_and_meta_kernel():
    assert mobile_vit.NATIVE_FFN is False  # opt-in
    a = ptq.arg_parser().parse_args(["mobilevit", "cifar10", "--data_file", "x", "--native-ffn"])
    assert a.native_ffn and not a.native_attention
    e = lambda *shape: torch.empty(shape, device="meta")  # noqa: E731
    for shape in ((17, 24), (2, 3, 17, 24)):
        y = _lib.ops().ffn(e(*shape), e(24), e(24), 1e-5, e(36, 24), e(36), e(24, 36), e(24), True, 0)
        assert y.device.type == "meta" and y.dtype == torch.float32 and tuple(y.shape) == shape


@pytest.mark.parametrize("over,msg", [({name: None}, b"null") for name in PTRS]
                         + [({"M": 0}, b"positive M"), ({"dim": 6}, b"dim = 6"), ({"dim": 4096}, b"dim = 4096"),
                            ({"hidden": 6}, b"hidden = 6"), ({"kernel": 3}, b"unknown kernel"),
                            ({"out": "x"}, b"overlap")])
def test_c_abi_rejects_before_launch(over, msg):
    L = _lib.load()
    buf = torch.zeros(8 * 256)  # never dereferenced: every error returns before any launch
    a = {name: buf.data_ptr() + 1024 * i for i, name in enumerate(PTRS)}
    a.update(M=5, dim=8, hidden=20, kernel=0)
    a.update(over)
    if a["out"] == "x":
        a["out"] = a["x"]
    st = L.po2q_ffn_f32(a["x"], a["ln_w"], a["ln_b"], 1e-5, a["w1"], a["b1"], a["w2"], a["b2"], a["out"], a["M"],
                        a["dim"], a["hidden"], 1, a["kernel"], None)
    assert st == 1
    assert msg in L.po2q_last_error()


def test_torch_path_is_kept_on_cpu_under_grad_and_with_dropout(monkeypatch):
    torch.manual_seed(5)
    tr = mobile_vit.Transformer(24, 2, 4, 8, 48).eval()
    drop = mobile_vit.Transformer(24, 1, 4, 8, 48, dropout=0.25).train()
    x = torch.randn(2, 4, 9, 24)

    def run():
        torch.manual_seed(11)  # the dropout masks
        with torch.no_grad():
            return tr(x), drop(x)

    want = run()
    want_grad = tr(x)  # a gradient is being recorded
    monkeypatch.setattr(mobile_vit, "NATIVE_FFN", True)
    monkeypatch.setattr(_lib, "ffn", lambda *a, **k: pytest.fail("the torch path reached the native kernel"))
    assert all(torch.equal(g, w) for g, w in zip(run(), want))
    got = tr(x)
    assert got.requires_grad and torch.equal(got.detach(), want_grad.detach())
