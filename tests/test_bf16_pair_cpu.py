"""No device: the bf16 conv pair's planning entries (po2q_qconv2d_pair_bf16_supported / _workspace_bytes /
_describe), the op's Meta kernel, the ptq option, and the model switch on a CPU forward.  (tests/test_capi.py
compares _lib.EXPORTS, which carries the four new names, with the header.)"""
import re

import pytest
import torch

from po2_quantization_amd import _lib, ptq
from po2_quantization_amd.models import quantized_conv as qc
from po2_quantization_amd.models.model import get_model
from po2_quantization_amd.utils.quantizers import quantizer_dict

# [max|w| partials 1 KiB][fragments 3 tap rows x k-steps x C / 16 tiles x 64 lanes x 16 bytes], twice
WS = {16: 2 * (1024 + 3 * 2 * 1 * 1024), 32: 2 * (1024 + 3 * 3 * 2 * 1024)}
ELIGIBLE = [(1, 16, 1, 2), (256, 16, 224, 224), (1, 16, 3, 256), (256, 32, 112, 112), (1, 32, 9, 128), (3, 32, 5, 70)]
NEIGHBOURS = [((2, 24, 9, 18), 1), ((2, 64, 9, 18), 1), ((2, 16, 9, 17), 1), ((1, 16, 3, 258), 1), ((1, 32, 3, 130), 1),
              ((2, 16, 9, 18), 3), ((2, 16, 9, 18), 4)]  # C = 24, C = 64, odd W, W past Wmax at either C, lin, lin+


@pytest.mark.parametrize("shape", ELIGIBLE, ids=str)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_eligible_shapes(shape, mode):
    L = _lib.load()
    assert L.po2q_qconv2d_pair_bf16_supported(*shape, 4, 1, mode) == 1
    assert L.po2q_qconv2d_pair_bf16_workspace_bytes(*shape, 4, 1, mode) == WS[shape[1]]
    N, C, H, W = shape
    m = re.match(r"kind=bf16_pair C=(\d+) RB=(\d+) bands=(\d+) groups=(\d+) GW=(\d+) lds=(\d+) blocks=(\d+)$",
                 _lib.describe_pair_bf16(*shape, mode=("none", "po2", "po2+")[mode]))
    c, rb, bands, groups, gw, lds, blocks = map(int, m.groups())
    assert (c, groups, bands, blocks) == (C, (W + 15) // 16, -(-H // rb), N * -(-H // rb)) and rb in (4, 8, 16)
    assert gw in (1, 2, 4) and 4 * gw >= groups and (gw == 1 or 2 * gw < groups) and (C == 16 or gw <= 2)
    assert lds == 6 * ((W + 2) * 2 * C + 16) + 4 * C * (32 * gw + 16) + 12 * C <= 64 * 1024


@pytest.mark.parametrize("shape,mode", NEIGHBOURS, ids=str)
def test_neighbours_are_unsupported(shape, mode):
    L = _lib.load()
    assert L.po2q_qconv2d_pair_bf16_supported(*shape, 4, 1, mode) == 0
    assert L.po2q_qconv2d_pair_bf16_workspace_bytes(*shape, 4, 1, mode) == 0
    buf = torch.zeros(8, dtype=torch.int16)  # never dereferenced: every error returns before any launch
    p = buf.data_ptr()
    st = L.po2q_qconv2d_pair_bf16(p, p, p, p + 2, *shape, 4, 1, mode, None, None, None, None, 1, None, None, 1, 1, p, 1 << 20,
                                  None)
    assert st == 2 and L.po2q_last_error()  # PO2Q_ERR_UNSUPPORTED
    assert not _lib.pair_bf16_supported(shape, 4, ("none", "po2", "po2+", "lin", "lin+")[mode])


def test_meta_kernel_and_ptq_option():
    x = torch.empty(2, 16, 8, 8, dtype=torch.bfloat16, device="meta")
    w = torch.empty(16, 16, 3, 3, dtype=torch.bfloat16, device="meta")
    y = _lib.ops().qconv2d_pair_bf16(x, w, w, None, None, 4, 1, 1, None, None, 1, None, None, True, 1)
    assert y.device.type == "meta" and y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 16, 8, 8)
    a = ptq.arg_parser().parse_args(["resnet20", "cifar10", "--data_file", "x", "--dtype", "bf16", "--bf16-fused-epilogue",
                                     "--bf16-pairs"])
    assert a.bf16_pairs and a.bf16_fused_epilogue
    assert qc.BF16_PAIRS is False  # opt-in


def test_cpu_forward_is_unchanged_with_the_switches_on(monkeypatch):
    torch.manual_seed(3)
    model = get_model("resnet20", 10, quantizer_dict["po2"], 4, (32, 32)).eval().bfloat16()
    x = torch.randn(2, 3, 32, 32).bfloat16()
    with torch.no_grad():
        want = model(x)
        monkeypatch.setattr(qc, "BF16_FUSED_EPILOGUE", True)
        monkeypatch.setattr(qc, "BF16_PAIRS", True)
        got = model(x)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
