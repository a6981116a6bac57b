"""No device: the projection switch's default, the ptq option, the op's Meta kernel, the host-side argument checks of
po2q_ln_linear_f32 and torch.ops.po2q.ln_linear, and the torch path of Attention / Transformer.forward with the switch
on (CPU tensors, recorded gradients, dropout)."""
import pytest
import torch

from po2_quantization_amd import _lib, ptq
from po2_quantization_amd.models import mobile_vit

PTRS = ("x", "ln_w", "ln_b", "w", "bias", "residual", "out")


def meta(*shape, dtype=torch.float32):
    return torch.empty(shape, device="meta", dtype=dtype)


def test_switch_default_ptq_option_and_meta_kernel():
    assert mobile_vit.NATIVE_PROJ is False  # opt-in
    a = ptq.arg_parser().parse_args(["mobilevit", "cifar10", "--data_file", "x", "--native-proj"])
    assert a.native_proj and not a.native_attention and not a.native_ffn
    for shape in ((17, 24), (2, 3, 17, 24)):
        out_shape = shape[:-1] + (36,)
        for y in (_lib.ops().ln_linear(meta(*shape), meta(24), meta(24), 1e-5, meta(36, 24), None, None, 0),
                  _lib.ops().ln_linear(meta(*shape), None, None, 1e-5, meta(36, 24), meta(36), meta(*out_shape), 0)):
            assert y.device.type == "meta" and y.dtype == torch.float32 and tuple(y.shape) == out_shape


@pytest.mark.parametrize("over,msg", [({name: None}, b"null") for name in ("x", "w", "out")]
                         + [({"ln_w": None}, b"together"), ({"ln_b": None}, b"together"), ({"M": 0}, b"positive M"),
                            ({"in_dim": 6}, b"in_dim = 6"), ({"in_dim": 644}, b"in_dim = 644"),
                            ({"out_dim": 6}, b"out_dim = 6"), ({"kernel": 3}, b"unknown kernel"),
                            ({"bias": 4}, b"aligned"), ({"out": "x"}, b"overlap"), ({"out": "residual"}, b"overlap")])
def test_c_abi_rejects_before_launch(over, msg):
    L = _lib.load()
    buf = torch.zeros(8 * 256)  # never dereferenced: every error returns before any launch
    a = {name: buf.data_ptr() + 1024 * i for i, name in enumerate(PTRS)}
    a.update(M=5, in_dim=8, out_dim=20, kernel=0)
    a.update(over)
    if a["out"] in a:
        a["out"] = a[a["out"]]
    if a["bias"] == 4:
        a["bias"] = buf.data_ptr() + 4
    st = L.po2q_ln_linear_f32(a["x"], a["ln_w"], a["ln_b"], 1e-5, a["w"], a["bias"], a["residual"], a["out"], a["M"],
                              a["in_dim"], a["out_dim"], a["kernel"], None)
    assert st == 1
    assert msg in L.po2q_last_error()


@pytest.mark.parametrize("over,msg", [({"ln_b": None}, "together"), ({"x": meta(5, 8, dtype=torch.float64)}, "float32"),
                                      ({"w": meta(20, 12)}, "w must be"), ({"bias": meta(8)}, "bias must hold"),
                                      ({"residual": meta(5, 8)}, "residual must be"),
                                      ({"ln_w": meta(20)}, "in_dim = 8")])
def test_op_rejects_mis_typed_and_mis_shaped_tensors(over, msg):
    a = dict(x=meta(5, 8), ln_w=meta(8), ln_b=meta(8), w=meta(20, 8), bias=meta(20), residual=meta(5, 20))
    a.update(over)
    with pytest.raises(RuntimeError, match=msg):
        _lib.ops().ln_linear(a["x"], a["ln_w"], a["ln_b"], 1e-5, a["w"], a["bias"], a["residual"], 0)


def test_torch_path_is_kept_on_cpu_under_grad_and_with_dropout(monkeypatch):
    torch.manual_seed(5)
    tr = mobile_vit.Transformer(24, 2, 4, 8, 48).eval()
    drop = mobile_vit.Transformer(24, 1, 4, 8, 48, dropout=0.25).train()
    x = torch.randn(2, 4, 9, 24)

    def run():
        torch.manual_seed(11)  # the dropout masks
        with torch.no_grad():
            return tr(x), drop(x), tr.layers[0][0](x)

    want = run()
    want_grad = tr(x)  # a gradient is being recorded
    monkeypatch.setattr(mobile_vit, "NATIVE_PROJ", True)
    monkeypatch.setattr(_lib, "ln_linear", lambda *a, **k: pytest.fail("the torch path reached the native kernel"))
    assert all(torch.equal(g, w) for g, w in zip(run(), want))
    got = tr(x)
    assert got.requires_grad and torch.equal(got.detach(), want_grad.detach())
