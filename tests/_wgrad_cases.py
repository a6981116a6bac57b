"""Shapes and helpers shared by the weight-gradient tests (tests/test_wgrad_cases_cpu.py,
tests/test_gpu_wgrad_paths.py, tests/test_gpu_backward.py).

The weight gradient has three kernels and no plan override a test may use: the register-streaming
wgrad2_f32<R, S, SH, PW, KW, CW, VEC> (32 instances), the LDS-band wgrad_f32<R, S> and the depthwise
dw_wgrad_partial<RS>.  Which instance, segment length, band height or slice count a layer gets is
decided by host heuristics, so coverage is pinned through the shapes below: the CPU test asks
describe_wgrad which kernel and plan each shape runs and fails when an instance or a named condition
is no longer reached; the GPU tests run every shape.

Fields: (N, C, H, W, K, R, S, sh, sw, ph, pw, dh, dw); groups is 1 for the dense tables and C for
DEPTHWISE (there K == C)."""
import re

import torch
import torch.nn.functional as F

from po2_quantization_amd import _lib

# ---- streaming grid: one shape per wgrad2_f32 instance -----------------------------------------
# K 16 / 40 -> KW 1 / 2, C 8 / 24 -> CW 1 / 2 (both ragged in their last 16-group), 3x3 pad 1 / 1x1
# pad 0, stride 1 / 2, and an image whose W and Q are multiples of 4 (vec) or not.  N = 3 gives
# items = 18 (stride 1) or 6 (stride 2): the last block of each channel group is partial.
_GRID_IMAGES = {(1, 1): (10, 24), (2, 1): (9, 24), (1, 0): (9, 21), (2, 0): (10, 23)}  # (stride, vec) -> H, W
STREAM_GRID = [(3, c, *_GRID_IMAGES[(st, vec)], k, r, r, st, st, r // 2, r // 2, 1, 1)
               for r in (3, 1) for st in (1, 2) for k in (16, 40) for c in (8, 24) for vec in (1, 0)]

# ---- streaming edges ---------------------------------------------------------------------------
LONG_RING = (4, 64, 250, 16, 512, 3, 3, 1, 1, 1, 1, 1, 1)      # 4096 waves: RB = 8, 32 segments, the last 2 rows
LONG_TWO_SLOT = (4, 64, 499, 31, 512, 3, 3, 2, 2, 1, 1, 1, 1)  # stride 2, P = 250: the two-slot loop, 4 turns
LONG_1X1 = (4, 64, 250, 16, 512, 1, 1, 1, 1, 0, 0, 1, 1)       # the 1x1 form of the two-slot loop
LONG = [LONG_RING, LONG_TWO_SLOT, LONG_1X1]
STREAM_EDGES = LONG + [
    (5, 16, 37, 70, 16, 3, 3, 1, 1, 1, 1, 1, 1),   # bpg = 63: wgrad2_reduce's slice loop runs 4 times
    (2, 16, 12, 12, 16, 3, 3, 1, 1, 0, 0, 1, 1),   # 3x3 padding 0 (pw != 1: scalar loads)
    (2, 16, 12, 12, 16, 3, 3, 1, 1, 2, 2, 1, 1),   # 3x3 padding 2
    (2, 16, 13, 13, 16, 3, 3, 2, 2, 0, 0, 1, 1),   # stride 2, padding 0
    (2, 16, 3, 20, 16, 3, 3, 1, 1, 1, 1, 1, 1),    # P = 3 < 4: the segment's last row is masked
    (2, 16, 20, 3, 16, 3, 3, 1, 1, 1, 1, 1, 1),    # Q = 3 < 4
    (2, 3, 16, 16, 16, 3, 3, 1, 1, 1, 1, 1, 1),    # C = 3
]
STREAM = STREAM_GRID + STREAM_EDGES

# ---- LDS-band cases: dilation != 1, unequal strides, stride >= 3 -------------------------------
BAND = [
    (2, 20, 12, 70, 40, 3, 3, 1, 1, 2, 2, 2, 2),   # 2 column tiles, the last 6 wide; BP 5 over P 12; KT 3, CT 2 ragged
    (3, 16, 20, 64, 16, 3, 3, 1, 1, 5, 5, 5, 5),   # BP = 1
    (2, 24, 16, 17, 16, 1, 1, 3, 3, 0, 0, 1, 1),   # wgrad_f32<1, 1>
    (2, 16, 13, 18, 24, 3, 3, 2, 1, 1, 1, 1, 1),   # stride (2, 1)
    (2, 16, 13, 18, 24, 3, 3, 1, 2, 1, 1, 1, 1),   # stride (1, 2)
    (2, 16, 17, 19, 16, 3, 3, 3, 3, 1, 1, 1, 1),   # stride 3
    (2, 16, 14, 16, 16, 3, 3, 1, 1, 2, 1, 2, 1),   # dilation (2, 1)
    (2, 16, 14, 16, 16, 3, 3, 1, 1, 1, 3, 1, 3),   # dilation (1, 3)
    (2, 16, 5, 10, 16, 3, 3, 1, 1, 0, 2, 2, 2),    # P = 1: 3 chunks for 4 waves
]

# ---- no plan: the band of a 3x3 with dilation >= 6 and Q >= 64 exceeds LDS at BP = 1 -----------
NO_PLAN_D6 = (1, 16, 64, 64, 16, 3, 3, 1, 1, 6, 6, 6, 6)
NO_PLAN = [NO_PLAN_D6, (1, 16, 64, 64, 16, 3, 3, 1, 1, 8, 8, 8, 8)]

# ---- depthwise cases (groups = C = K) ----------------------------------------------------------
DEPTHWISE = [
    (9, 8, 32, 32, 8, 3, 3, 1, 1, 1, 1, 1, 1),     # nslice = 2, per_slice = 5: the last slice has 4 images
    (2, 8, 12, 14, 8, 3, 5, 1, 1, 1, 2, 1, 1),     # 3x5 through the 25-tap instance
    (2, 8, 12, 14, 8, 7, 3, 1, 1, 3, 1, 1, 1),     # 7x3
    (1, 24, 9, 13, 24, 5, 5, 1, 1, 2, 2, 1, 1),    # 5x5
    (2, 8, 6, 6, 8, 1, 1, 1, 1, 0, 0, 1, 1),       # 1x1
    (2, 8, 13, 12, 8, 3, 3, 2, 1, 0, 2, 2, 1),     # stride (2, 1), padding (0, 2), dilation (2, 1)
    (2, 16, 5, 7, 16, 3, 3, 1, 1, 1, 1, 1, 1),     # P * Q = 35: most of the block has no pixel
]
DEPTHWISE_UNSUPPORTED = (1, 16, 9, 9, 16, 1, 7, 1, 1, 0, 3, 1, 1)  # S > 5

# ---- alignment: vec = 1 shapes run from buffers 4, 8 and 12 bytes past a 16-byte boundary ------
ALIGNMENT = [
    (3, 8, 10, 24, 16, 3, 3, 1, 1, 1, 1, 1, 1),
    (3, 24, 9, 24, 40, 1, 1, 2, 2, 0, 0, 1, 1),
]

# every case the GPU tests run: (shape, groups)
RUN = [(s, 1) for s in STREAM + BAND] + [(s, s[1]) for s in DEPTHWISE]


def case_id(shape):
    return "x".join(map(str, shape))


def conv_args(shape):
    """(stride, padding, dilation) pairs of a 13-field case."""
    return (shape[7], shape[8]), (shape[9], shape[10]), (shape[11], shape[12])


def out_size(shape):
    N, C, H, W, K, R, S, sh, sw, ph, pw, dh, dw = shape
    return (H + 2 * ph - dh * (R - 1) - 1) // sh + 1, (W + 2 * pw - dw * (S - 1) - 1) // sw + 1


def wshape(shape, groups=1):
    return (shape[4], shape[1] // groups, shape[5], shape[6])


def describe(shape, groups=1):
    stride, pad, dil = conv_args(shape)
    return _lib.describe_wgrad(*shape[:7], stride, pad, dil, groups)


def parse(desc):
    """describe_wgrad's line -> (kind, {field: int})."""
    m = re.match(r"kind=(\w+)((?: \w+=\d+)+)$", desc)
    assert m, "not a wgrad description: %r" % desc
    return m.group(1), {k: int(v) for k, v in (f.split("=") for f in m.group(2).split())}


# ---- operands and references ---------------------------------------------------------------------
def operands(shape, seed, exact):
    """(x, gy) on the CPU: integers in [-4, 4] (exact) or standard normal."""
    N, C, H, W, K = shape[:5]
    P, Q = out_size(shape)
    g = torch.Generator().manual_seed(seed)
    if exact:
        return (torch.randint(-4, 5, (N, C, H, W), generator=g).float(),
                torch.randint(-4, 5, (N, K, P, Q), generator=g).float())
    return torch.randn(N, C, H, W, generator=g), torch.randn(N, K, P, Q, generator=g)


def reference_cpu(x, gy, shape, groups=1):
    """The weight gradient by aten.convolution_backward in fp64 on the CPU."""
    stride, pad, dil = conv_args(shape)
    w0 = torch.zeros(wshape(shape, groups), dtype=torch.float64)
    _, rw, _ = torch.ops.aten.convolution_backward(gy.double().cpu(), x.double().cpu(), w0, None, list(stride),
                                                   list(pad), list(dil), False, [0, 0], groups, [False, True, False])
    return rw


def reference_unfold(x, gy, shape):
    """The dense weight gradient in fp64 on x's device as unfold(x) times gy (plain torch ops, no library
    code), for the cases whose CPU reference would take too long.  Pinned against reference_cpu in
    tests/test_gpu_wgrad_paths.py."""
    stride, pad, dil = conv_args(shape)
    cols = F.unfold(x.double(), (shape[5], shape[6]), dilation=dil, padding=pad, stride=stride)  # [N, C R S, P Q]
    rw = torch.einsum("nkl,ncl->kc", gy.double().flatten(2), cols)
    return rw.view(wshape(shape)).cpu()


def exact_sums_fit(shape):
    """Every partial sum of products of integers in [-4, 4] over (n, p, q), in any order, is an integer
    below 2^24: exact in fp32."""
    P, Q = out_size(shape)
    return 16 * shape[0] * P * Q < 2 ** 24
