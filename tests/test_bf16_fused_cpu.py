"""CPU: what the fused bf16 conv entry (po2q_qconv2d_fused_bf16) adds and can be checked without a GPU:
the exported symbol, the torch op's schema and Meta kernel, the opt-in switch, the fp32 fold of a bf16
BatchNorm and the evaluation harness's flag."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from po2_quantization_amd import _lib
from po2_quantization_amd.models import quantized_conv as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry():
    L = ctypes.CDLL(os.path.join(ROOT, "po2_quantization_amd", "lib", "libpo2q.so"))
    assert hasattr(L, "po2q_qconv2d_fused_bf16")
    assert "po2q_qconv2d_fused_bf16" in _lib.EXPORTS
    assert "po2q_qconv2d_fused_bf16" in open(os.path.join(ROOT, "include", "po2q.h")).read()
    assert callable(_lib.qconv2d_fused_bf16)


def test_op_schema():
    assert _lib.ops() is not None
    schema = str(torch.ops.po2q.qconv2d_fused_bf16.default._schema)
    for arg in ("Tensor x", "Tensor w", "Tensor? bias", "int[] stride", "int[] padding", "int[] dilation",
                "int groups", "int bits", "int mode", "int fsr", "Tensor? post_scale", "Tensor? post_shift",
                "Tensor? residual", "int act"):
        assert arg in schema, (arg, schema)
    assert schema.endswith("-> Tensor")


@pytest.mark.parametrize("shape,conv,want", [
    ((2, 16, 9, 10), (24, 3, 1, 1), (2, 24, 9, 10)),     # dense 3x3
    ((1, 20, 11, 15), (24, 3, 2, 1), (1, 24, 6, 8)),     # stride 2
], ids=["dense", "stride2"])
def test_meta_kernel(shape, conv, want):
    _lib.ops()
    K, R, stride, pad = conv
    x = torch.empty(shape, dtype=torch.bfloat16, device="meta")
    w = torch.empty(K, shape[1], R, R, dtype=torch.bfloat16, device="meta")
    s = torch.empty(K, dtype=torch.float32, device="meta")
    r = torch.empty(want, dtype=torch.bfloat16, device="meta")
    y = torch.ops.po2q.qconv2d_fused_bf16(x, w, None, [stride, stride], [pad, pad], [1, 1], 1, 4, 1, 1, s, s, r, 1)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == want and y.device.type == "meta"


def test_switch_exists_and_is_off():
    assert qc.BF16_FUSED_EPILOGUE is False
    x = torch.zeros(1, 3, 4, 4, dtype=torch.bfloat16)
    assert not qc.bf16_fused_input(x)


def _bn(affine=True):
    torch.manual_seed(5)
    bn = nn.BatchNorm2d(24, affine=affine)
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        if affine:
            bn.weight.normal_()
            bn.bias.normal_()
    return bn.eval()


@pytest.mark.parametrize("affine", [True, False])
def test_fp32_fold_of_a_bf16_batchnorm(affine):
    bn = _bn(affine).bfloat16()
    up = nn.BatchNorm2d(24, affine=affine).eval()  # the same module's parameters upcast to fp32
    up.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    s, t = qc.fold_bn_f32(bn)
    ws, wt = qc.fold_bn(up)
    assert s.dtype == torch.float32 and t.dtype == torch.float32
    assert torch.equal(s, ws) and torch.equal(t, wt)
    # cached, under a key of its own: the module-dtype fold next to it does not disturb it
    s16, t16 = qc.fold_bn(bn)
    assert s16.dtype == torch.bfloat16
    s2, t2 = qc.fold_bn_f32(bn)
    assert s2 is s and t2 is t and qc.fold_bn(bn)[0] is s16
    with torch.no_grad():
        bn.running_var.mul_(2.0)  # an in-place update changes the key
    s3, _ = qc.fold_bn_f32(bn)
    assert s3 is not s and not torch.equal(s3, s)


def test_fold_bn_of_an_fp32_batchnorm_is_unchanged():
    bn = _bn()
    s, t = qc.fold_bn(bn)
    want_s = torch.rsqrt(bn.running_var + bn.eps) * bn.weight  # the formula of fold_bn's docstring
    want_t = bn.bias - bn.running_mean * want_s
    assert s.dtype == torch.float32 and torch.equal(s, want_s.detach()) and torch.equal(t, want_t.detach())
    s32, t32 = qc.fold_bn_f32(bn)  # an fp32 module: fold_bn's own tensors
    assert s32 is s and t32 is t


def test_ptq_help_lists_the_flag():
    out = subprocess.run([sys.executable, "-m", "po2_quantization_amd.ptq", "--help"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--bf16-fused-epilogue" in out.stdout
