"""Shapes and helpers shared by the bf16 conv tests (tests/test_bf16_conv_cpu.py,
tests/test_gpu_bf16_conv.py, tests/test_gpu_bf16_conv_paths.py).

The bf16 forward has one heuristic planner and no plan override, so coverage of its 18
conv_bf16x1<CC, NT, NJ> instances, of its staging (dword "pair" / 2-byte) and store (8-byte /
2-byte) paths and of its block decomposition is pinned through the shapes below: the CPU test asks
describe_bf16 which kernel each shape runs and fails when an instance or a named condition is no
longer reached; the GPU tests run every shape.

The error bar and the exact operands are the ones derived in tests/test_gpu_bf16_conv.py's
docstring; this module only carries them, for square and rectangular kernels alike."""
import collections
import re

import torch
import torch.nn.functional as F

from po2_quantization_amd import _lib

BF = torch.bfloat16
BITS = 4
MODES = ["po2", "po2+", "none"]

# ---- dense cases: (N, C, H, W, K, R, S, sh, sw, ph, pw, dh, dw), groups = 1 --------------------
# Instance grid: 1x1 convs at stride 1, pad 0.  C 16 / 24 -> CC 16 / 32, K 16 / 24 / 48 -> NT 1 / 2 / 4,
# and four geometries -> NJ 1 (a tile far larger than the image), NJ 2 (odd W: 2-byte staging),
# NJ 4 (several tiles with a ragged last Q tile, pair staging), NJ 2 with a 64x2 tile (2-byte stores).
GRID_GEOMETRIES = [(1, 3, 2), (1, 5, 9), (1, 40, 66), (1, 33, 2)]
GRID = [(n, c, h, w, k, 1, 1, 1, 1, 0, 0, 1, 1)
        for c in (16, 24) for k in (16, 24, 48) for (n, h, w) in GRID_GEOMETRIES]

EDGES = [
    (3, 16, 9, 10, 80, 3, 3, 1, 1, 1, 1, 1, 1),    # 2 k-blocks, the last with 16 of 64 channels; N = 3
    (2, 40, 6, 10, 80, 3, 3, 1, 1, 1, 1, 1, 1),    # 2 k-blocks x 3 chunks, ragged last chunk
    (2, 8, 9, 11, 64, 5, 5, 1, 1, 2, 2, 1, 1),     # NT halved 4 -> 1, 4 k-blocks, 13 k-steps, C < CC
    (1, 24, 13, 12, 24, 7, 7, 1, 1, 3, 3, 1, 1),   # 25 k-steps, 2 chunks, 2 k-blocks
    (1, 16, 9, 9, 16, 9, 9, 1, 1, 4, 4, 1, 1),     # the largest kernel that fits LDS
    (1, 16, 70, 2, 16, 3, 3, 1, 1, 1, 1, 1, 1),    # 2-byte stores with a 3x3 halo, several P tiles
    (2, 16, 9, 70, 16, 3, 3, 1, 1, 1, 1, 1, 1),    # pair staging, several Q tiles, odd w0, ragged last tile
    (2, 16, 9, 71, 16, 3, 3, 1, 1, 1, 1, 1, 1),    # the same with odd W: 2-byte staging, odd output rows
    (2, 16, 40, 66, 16, 3, 3, 1, 1, 1, 1, 1, 1),   # NJ 4 with a 3x3 halo, tiles in both directions
    (1, 16, 19, 70, 24, 3, 3, 2, 2, 1, 1, 1, 1),   # stride 2 with pair staging, Q = 35
    (1, 20, 12, 14, 24, 3, 5, 1, 1, 1, 2, 1, 1),   # R != S, 15 taps (padded k-slots), 2 chunks
    (1, 20, 12, 14, 24, 5, 3, 2, 1, 2, 1, 1, 1),   # R != S transposed, stride (2, 1)
    (1, 16, 12, 14, 16, 3, 3, 1, 2, 0, 2, 1, 1),   # stride (1, 2), pad (0, 2)
    (1, 16, 14, 16, 16, 3, 3, 1, 1, 2, 1, 2, 1),   # dilation (2, 1)
    (1, 16, 14, 16, 16, 3, 3, 1, 1, 1, 2, 1, 2),   # dilation (1, 2)
    (1, 16, 14, 16, 16, 3, 3, 2, 2, 3, 3, 3, 3),   # dilation 3 with stride 2
    (1, 40, 9, 10, 16, 1, 1, 1, 2, 0, 0, 1, 1),    # CC = 32 with a ragged second chunk, stride (1, 2)
]
DENSE = GRID + EDGES

# ---- depthwise cases, the same 13 fields with K = C; groups = C --------------------------------
DEPTHWISE = [
    (2, 24, 9, 11, 24, 3, 5, 1, 2, 1, 2, 1, 1),
    (1, 16, 12, 10, 16, 5, 5, 2, 2, 2, 2, 1, 1),
    (1, 8, 11, 11, 8, 3, 3, 1, 1, 2, 1, 2, 1),
    (3, 40, 1, 7, 40, 3, 3, 1, 1, 1, 1, 1, 1),
]

# Pointer-alignment cases: dword ("pair", even W) or 2-byte staging by 8-byte (TQ % 4 == 0) or 2-byte
# stores, as the run with aligned pointers takes them
ALIGNMENT = [
    (2, 16, 9, 70, 16, 3, 3, 1, 1, 1, 1, 1, 1),   # pair staging, 8-byte stores
    (2, 16, 9, 71, 16, 3, 3, 1, 1, 1, 1, 1, 1),   # 2-byte staging, 8-byte stores where a row start allows
    (1, 16, 70, 2, 16, 3, 3, 1, 1, 1, 1, 1, 1),   # pair staging, 2-byte stores
    (1, 16, 33, 3, 16, 3, 3, 1, 2, 1, 1, 1, 1),   # 2-byte staging, 2-byte stores (Q = 2)
]

# 11x11: no tile fits LDS; 9x9 (in EDGES) is the largest that does
TOO_LARGE = (1, 16, 11, 11, 16, 11, 11, 1, 1, 5, 5, 1, 1)
LARGEST = (1, 16, 9, 9, 16, 9, 9, 1, 1, 4, 4, 1, 1)


def case_id(shape):
    return "x".join(map(str, shape))


def conv_args(shape):
    """(stride, padding, dilation) pairs of a 13-field case."""
    return (shape[7], shape[8]), (shape[9], shape[10]), (shape[11], shape[12])


def out_size(shape):
    N, C, H, W, K, R, S, sh, sw, ph, pw, dh, dw = shape
    return (H + 2 * ph - dh * (R - 1) - 1) // sh + 1, (W + 2 * pw - dw * (S - 1) - 1) // sw + 1


def geom14(shape, groups=1):
    """The 14 geometry arguments of the C ABI."""
    return tuple(shape) + (groups,)


Plan = collections.namedtuple("Plan", "CC NT NJ TP TQ tilesP tilesQ chunks kblocks ksteps")
_PLAN_RE = re.compile(r"kind=bf16x1 CC=(\d+) NT=(\d+) NJ=(\d+) tile=(\d+)x(\d+) tiles=(\d+)x(\d+) halo=\d+x\d+ "
                      r"chunks=(\d+) kblocks=(\d+) ksteps=(\d+) lds=(\d+) ")


def parse_plan(desc):
    """describe_bf16's text of a dense conv -> (CC, NT, NJ, TP, TQ, tilesP, tilesQ, chunks, kblocks, ksteps)."""
    m = _PLAN_RE.match(desc)
    assert m, "not a bf16x1 description: %r" % desc
    return Plan(*map(int, m.groups()[:10]))


def parse_lds(desc):
    m = _PLAN_RE.match(desc)
    assert m, "not a bf16x1 description: %r" % desc
    return int(m.group(11))


def describe(shape, groups=1):
    stride, pad, dil = conv_args(shape)
    return _lib.describe_bf16(*shape[:7], stride, pad, dil, groups)


# ---- operands, reference and bar -----------------------------------------------------------------
def _kernel(shape):
    """(R, S): the 9-field shapes of tests/test_gpu_bf16_conv.py are square, the 13-field ones carry both."""
    return (shape[5], shape[6]) if len(shape) == 13 else (shape[5], shape[5])


def quantized(w, mode, bits=BITS, fsr=1):
    return w if mode == "none" else _lib.restated_quantize(w, bits, mode, fsr)


def reference(x, q, b, stride, pad, dil, groups):
    """(ref, mag) in fp64 on the CPU."""
    bd = b.double() if b is not None else None
    ref = F.conv2d(x.double(), q.double(), bd, stride, pad, dil, groups)
    mag = F.conv2d(x.double().abs(), q.double().abs(), bd.abs() if bd is not None else None, stride, pad, dil, groups)
    return ref, mag


def bar(ref, mag, k):
    return 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * (k + 3) * 2.0 ** -23 * mag


def assert_bar(y, ref, mag, k, what=""):
    tol = bar(ref, mag, k)
    err = (y.double().cpu() - ref).abs()
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    print("%s worst |y - ref| / bar = %.3f" % (what, ratio))
    assert torch.isfinite(y.float()).all(), what
    assert bool((err <= tol).all()), (what, ratio)


def random_case(shape, groups, seed, bias):
    N, C, H, W, K = shape[:5]
    R, S = _kernel(shape)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g).to(BF)
    w = (torch.randn(K, C // groups, R, S, generator=g) * 0.1).to(BF)
    b = torch.randn(K, generator=g).to(BF) if bias else None
    return x, w, b


def exact_case(shape, groups, seed, bias, mode):
    N, C, H, W, K = shape[:5]
    R, S = _kernel(shape)
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (N, C, H, W), generator=g).to(BF)
    if mode == "none":
        w = (torch.randint(-8, 9, (K, C // groups, R, S), generator=g).float() / 8).to(BF)
    else:  # one element 1.0, the rest in [-1, 1]: the scale is 1 and Q(w) a multiple of 2^-7
        w = (torch.rand(K, C // groups, R, S, generator=g) * 2 - 1).to(BF)
        w.view(-1)[0] = 1.0
    b = (torch.randint(-8, 9, (K,), generator=g).float() / 8).to(BF) if bias else None
    return x, w, b
