"""Shapes of the C = K = 64 bf16 row-streaming conv kernel's tests (tests/test_bf16_rowsk_cpu.py,
tests/test_gpu_bf16_rowsk.py): 13-field cases in the layout of tests/_bf16_cases.py, every one a
3x3 / stride 1 / pad 1 / dilation 1 layer with C == K == 64 and an even W <= Wmax = 64, i.e. eligible for
conv_b16_rowsk<GW, EPI> when its switch (po2q_bf16_set_rowsk_kernels) is on.

The planner gives a block RB output rows of one image across the whole width (RB = 16, halved down to
4 while the grid has fewer than 1024 blocks); wave w owns the output channels 16 w .. 16 w + 15 and
computes every 16-column group of the row, in GW = 1, 2 or 4 group slots.  The CPU test states the
conditions this table has to meet as predicates over the parsed description, so a planner change that
leaves one unmet fails there by name."""
import collections
import re

from tests import _bf16_cases as cases
from tests import _bf16_rows_cases as rc

WMAX = 64  # DESIGN.md "bf16 row kernel, C = 64": 4 group slots x 16 columns
C = 64

_c = rc._c

TABLE = [
    _c(1, 64, 1, 2),      # H = 1: both neighbour rows outside the image; W = 2: one group of 2 live columns
    _c(1, 64, 2, 8),      # H = 2
    _c(2, 64, 8, 8),      # ResNet20 stage 3; half-filled single group; GW = 1
    _c(1, 64, 4, 16),     # one exactly full group
    _c(2, 64, 9, 18),     # GW = 2; ragged second group; ragged last band (RB = 4, 9 rows)
    _c(1, 64, 7, 34),     # 3 groups in the GW = 4 instance: one group slot idle
    _c(3, 64, 5, 56),     # the ResNet56 @224 width: 3.5 groups; N = 3
    _c(1, 64, 3, 64),     # W = Wmax, all groups full
    _c(64, 64, 128, 2),   # RB = 8 (64 x 8 bands = 512 < 1024 <= 64 x 16)
    _c(128, 64, 129, 2),  # RB = 16 with a one-row last band (128 x 9 = 1152 blocks)
]

# One change away from an eligible layer: each is planned as with both switches off, whatever the new
# switch says.  (shape, groups, what)
INELIGIBLE = [
    ((2, 64, 9, 18, 64, 3, 3, 2, 2, 1, 1, 1, 1), 1, "stride 2"),
    ((2, 64, 9, 18, 64, 3, 3, 1, 1, 0, 0, 1, 1), 1, "pad 0"),
    ((2, 64, 9, 18, 64, 3, 3, 1, 1, 2, 2, 2, 2), 1, "dilation 2"),
    ((2, 64, 9, 18, 64, 3, 5, 1, 1, 1, 2, 1, 1), 1, "3x5 kernel"),
    ((2, 64, 9, 18, 64, 1, 1, 1, 1, 0, 0, 1, 1), 1, "1x1 kernel"),
    ((2, 64, 9, 18, 128, 3, 3, 1, 1, 1, 1, 1, 1), 1, "64 -> 128"),
    ((2, 32, 9, 18, 64, 3, 3, 1, 1, 1, 1, 1, 1), 1, "32 -> 64"),
    (_c(2, 48, 9, 18), 1, "C = 48"),
    (_c(2, 128, 9, 18), 1, "C = 128"),
    (_c(2, 64, 9, 17), 1, "odd W = 17"),
    (_c(1, 64, 3, WMAX + 2), 1, "W = 66"),
    (_c(2, 64, 9, 18), 64, "depthwise 64"),
    (_c(2, 16, 9, 18), 1, "C = 16 (the first switch's)"),
    (_c(2, 32, 9, 16), 1, "C = 32 (the first switch's)"),
]

RowsK = collections.namedtuple("RowsK", "C RB bands groups GW ring lds blocks")
_ROWSK_RE = re.compile(r"kind=bf16_rowsk C=(\d+) RB=(\d+) bands=(\d+) groups=(\d+) GW=(\d+) ring=(\d+) lds=(\d+) "
                       r"blocks=(\d+)$")


def parse_rowsk(desc):
    m = _ROWSK_RE.match(desc)
    assert m, "not a bf16_rowsk description: %r" % desc
    return RowsK(*map(int, m.groups()))


describe = rc.describe
workspace_bytes = rc.workspace_bytes


def is_rowsk(shape, groups=1):
    return describe(shape, groups).startswith("kind=bf16_rowsk ")


def all_shapes():
    """Every (shape, groups) this switch must leave alone while it is off."""
    return rc.golden_shapes() + [(s, 1) for s in TABLE] + [(s, g) for s, g, _ in INELIGIBLE]


def case_id(v):
    return cases.case_id(v) if isinstance(v, tuple) else str(v)
