"""Shapes of the bf16 row-streaming conv kernel's tests (tests/test_bf16_rows_cpu.py,
tests/test_gpu_bf16_rows.py): 13-field cases in the layout of tests/_bf16_cases.py, every one a
3x3 / stride 1 / pad 1 / dilation 1 layer with C == K in {16, 32} and an even W <= Wmax, i.e. eligible
for conv_b16_rows<C, GW, EPI> when the switch (po2q_bf16_set_row_kernels) is on.

The planner gives a block RB output rows of one image across the whole width (RB = 16, halved down to
4 while the grid has fewer than 1024 blocks) and deals the 16-column groups to 4 waves, GW = 1, 2 or 4
consecutive groups per wave.  The CPU test states the conditions this table has to meet as predicates
over the parsed description, so a planner change that leaves one unmet fails there by name."""
import collections
import json
import os
import re

from po2_quantization_amd import _lib
from tests import _bf16_cases as cases

WMAX = 256  # DESIGN.md "bf16 row kernel": 4 waves x 4 groups x 16 columns
WAVES = 4


def _c(n, c, h, w):
    return (n, c, h, w, c, 3, 3, 1, 1, 1, 1, 1, 1)


TABLE = [
    _c(2, 16, 1, 18),      # H = 1: two of three halo rows outside the image; W = 16 g + 2
    _c(2, 32, 2, 34),      # H = 2; 3 groups over 4 waves (one idle)
    _c(2, 16, 8, 32),      # H = 2 RB, W = 16 g: no ragged row band, no ragged group
    _c(3, 16, 9, 2),       # H = 2 RB + 1: a one-row last band; W = 2: a single masked group; N = 3
    _c(2, 32, 9, 16),      # the same band split at C = 32, one full group
    _c(1, 16, 3, WMAX),    # W = Wmax, H = 3: GW = 4, every wave full
    _c(1, 32, 3, WMAX),    # the same at C = 32 (the largest instance)
    _c(2, 16, 5, 82),      # 6 groups, GW = 2: waves 2 / 2 / 2 / 0, ragged last group
    _c(3, 32, 6, 50),      # C = 32, 4 groups (the last with 2 columns), bands of 4 and 2 rows; N = 3
    _c(2, 32, 4, 100),     # 7 groups, GW = 2: waves 2 / 2 / 2 / 1; H = RB
    _c(2, 16, 12, 130),    # 9 groups, GW = 4: waves 4 / 4 / 1 / 0; three bands
    _c(64, 16, 128, 2),    # 1024 blocks at RB = 8
    _c(128, 16, 129, 2),   # RB = 16 with a one-row last band
]

# One change away from an eligible layer: each keeps the tile / depthwise kernel whatever the switch says.
# (shape, groups, what)
INELIGIBLE = [
    ((2, 16, 9, 18, 16, 3, 3, 2, 2, 1, 1, 1, 1), 1, "stride 2"),
    ((2, 16, 9, 18, 16, 3, 3, 1, 1, 0, 0, 1, 1), 1, "pad 0"),
    ((2, 16, 9, 18, 16, 3, 3, 1, 1, 2, 2, 2, 2), 1, "dilation 2"),
    ((2, 16, 9, 18, 16, 3, 5, 1, 1, 1, 2, 1, 1), 1, "3x5 kernel"),
    ((2, 16, 9, 18, 16, 1, 1, 1, 1, 0, 0, 1, 1), 1, "1x1 kernel"),
    ((2, 16, 9, 18, 32, 3, 3, 1, 1, 1, 1, 1, 1), 1, "C != K"),
    (_c(2, 24, 9, 18), 1, "C = 24"),
    (_c(2, 64, 9, 18), 1, "C = 64"),
    (_c(2, 16, 9, 17), 1, "odd W"),
    (_c(1, 16, 3, WMAX + 2), 1, "W = Wmax + 2"),
    (_c(2, 16, 9, 18), 16, "depthwise"),
]

Rows = collections.namedtuple("Rows", "C RB bands groups ring lds blocks")
_ROWS_RE = re.compile(r"kind=bf16_rows C=(\d+) RB=(\d+) bands=(\d+) groups=(\d+) ring=(\d+) lds=(\d+) blocks=(\d+)$")


def parse_rows(desc):
    m = _ROWS_RE.match(desc)
    assert m, "not a bf16_rows description: %r" % desc
    return Rows(*map(int, m.groups()))


def describe(shape, groups=1):
    return cases.describe(shape, groups)


def workspace_bytes(shape, groups=1, bits=cases.BITS, fsr=1, mode=1):
    return _lib.load().po2q_qconv2d_bf16_workspace_bytes(*cases.geom14(shape, groups), bits, fsr, mode)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_rows_switch_off.json")


def golden_shapes():
    """Every (shape, groups) whose switch-off description and workspace size are pinned."""
    out = [(s, 1) for s in TABLE] + [(s, 1) for s in cases.DENSE] + [(s, s[1]) for s in cases.DEPTHWISE]
    out += [((2, 16, 10, 10, 16, 3, 3, 1, 1, 1, 1, 1, 1), 1), ((256, 16, 224, 224, 16, 3, 3, 1, 1, 1, 1, 1, 1), 1)]
    out += [(s, g) for s, g, _ in INELIGIBLE]
    return out


def load_golden():
    with open(GOLDEN) as f:
        return {(tuple(e["shape"]), e["groups"]): (e["describe"], e["workspace_bytes"]) for e in json.load(f)}
