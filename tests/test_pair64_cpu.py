"""Host-side contract of the chain entry's second geometry (large C = 64 images: ResNet56 stage 3 at
56 x 56, run as conv_pair64 launches): which shapes po2q_qconv2d_chain_supported takes, the
PO2Q_PAIR64=0 switch, the workspace query, and the unchanged per-block pair advice.  No GPU."""
import pytest

from po2_quantization_amd import _lib

YES = [((256, 64, 56, 56), 17), ((2, 64, 5, 36), 2)]
NO = [((256, 64, 16, 16), 4),     # CIFAR stage 3 at bs 256 stays with the single-conv path
      ((256, 16, 224, 224), 18),  # stage 1
      ((256, 32, 112, 112), 17),  # stage 2
      ((2, 64, 8, 58), 4),        # W % 4 != 0
      ((2, 64, 8, 68), 4),        # W > 64
      ((2, 64, 8, 56), 25),       # more than PO2Q_CHAIN_MAX_LAYERS
      ((2, 64, 8, 56), 1)]        # a single layer is no run


def ws_bytes(shape, n):
    return int(_lib.load().po2q_qconv2d_chain_workspace_bytes(*shape, n))


@pytest.mark.parametrize("shape,n", YES, ids=[str(c) for c in YES])
def test_large_c64_runs_supported(shape, n):
    for mode in ("po2", "po2+"):
        assert _lib.chain_supported(shape, n, 4, mode)
    assert not _lib.chain_supported(shape, n, 4, "none")
    N, C, H, W = shape
    # the packs of every layer and two activation buffers
    assert ws_bytes(shape, n) >= 2 * 4 * N * C * H * W + n * 3 * 6 * 4 * 64 * 16


@pytest.mark.parametrize("shape,n", NO, ids=[str(c) for c in NO])
def test_other_shapes_answer_as_before(shape, n):
    assert not _lib.chain_supported(shape, n, 4, "po2")
    assert ws_bytes(shape, n) == 0


def test_small_image_chain_unchanged():
    assert _lib.chain_supported((256, 64, 8, 8), 17, 4, "po2")
    assert _lib.chain_supported((256, 16, 32, 32), 18, 4, "po2")
    assert ws_bytes((256, 64, 8, 8), 17) > 0


def test_pair64_switch_off(monkeypatch):
    monkeypatch.setenv("PO2Q_PAIR64", "0")
    for shape, n in YES + NO:
        assert not _lib.chain_supported(shape, n, 4, "po2")
        assert ws_bytes(shape, n) == 0
    assert _lib.chain_supported((256, 64, 8, 8), 17, 4, "po2")  # the one-launch geometry does not depend on it
    monkeypatch.setenv("PO2Q_PAIR64", "1")
    assert _lib.chain_supported(*YES[0], 4, "po2")


def test_workspace_positive_exactly_where_supported():
    for shape, n in YES + NO + [((256, 64, 8, 8), 17), ((4, 64, 3, 36), 2), ((1, 64, 1, 64), 24)]:
        assert (ws_bytes(shape, n) > 0) == _lib.chain_supported(shape, n, 4, "po2")


def test_pair_advice_unchanged():
    assert not _lib.pair_supported((256, 64, 56, 56))
    assert not _lib.pair_supported((2, 64, 7, 64))
