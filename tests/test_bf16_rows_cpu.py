"""Host side of the bf16 row-streaming conv kernel (conv_b16_rows, "kind=bf16_rows"): the opt-in switch,
the planner with the switch off and on, the eligibility boundary and the case table's coverage.  Needs
the built library, no device.

With the switch off nothing may differ from the library before the kernel existed: the descriptions and
workspace sizes of tests/golden/bf16_rows_switch_off.json were written by that library."""
import os
import subprocess
import sys

import pytest
import torch

from po2_quantization_amd import _lib, ptq
from tests import _bf16_cases as cases
from tests import _bf16_rows_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def switch_off_around_each_test():
    prev = _lib.set_bf16_row_kernels(False)
    yield
    _lib.set_bf16_row_kernels(prev)


# ---- the switch ------------------------------------------------------------------------------------
def test_symbols_exported():
    L = _lib.load()
    for name in ("po2q_bf16_set_row_kernels", "po2q_bf16_row_kernels"):
        assert hasattr(L, name) and name in _lib.EXPORTS


def _child(env_value, code):
    env = dict(os.environ)
    env.pop("PO2Q_B16_ROWS", None)
    if env_value is not None:
        env["PO2Q_B16_ROWS"] = env_value
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.strip()


def test_switch_defaults_to_off_and_follows_the_environment_in_a_fresh_process():
    code = ("from po2_quantization_amd import _lib\n"
            "print(int(_lib.bf16_row_kernels()), _lib.describe_bf16(2, 16, 9, 18, 16, 3, 3, 1, 1).split()[0])")
    assert _child(None, code) == "0 kind=bf16x1"
    assert _child("0", code) == "0 kind=bf16x1"
    assert _child("1", code) == "1 kind=bf16_rows"


def test_setter_returns_the_previous_value():
    assert _lib.bf16_row_kernels() is False
    assert _lib.set_bf16_row_kernels(True) is False
    assert _lib.bf16_row_kernels() is True
    assert _lib.set_bf16_row_kernels(True) is True
    assert _lib.set_bf16_row_kernels(False) is True
    assert _lib.bf16_row_kernels() is False
    L = _lib.load()
    assert L.po2q_bf16_set_row_kernels(7) == 0 and L.po2q_bf16_row_kernels() == 1  # any non-zero value: on
    assert L.po2q_bf16_set_row_kernels(0) == 1


def test_context_manager_restores_the_previous_value():
    with _lib.bf16_rows():
        assert _lib.bf16_row_kernels()
        with _lib.bf16_rows(False):
            assert not _lib.bf16_row_kernels()
        assert _lib.bf16_row_kernels()
    assert not _lib.bf16_row_kernels()
    with pytest.raises(ZeroDivisionError):
        with _lib.bf16_rows():
            1 / 0
    assert not _lib.bf16_row_kernels()


# ---- switch off: the parent's planner, byte for byte -------------------------------------------------
def test_golden_list_covers_every_pinned_shape():
    assert set(rc.load_golden()) == set(rc.golden_shapes())


@pytest.mark.parametrize("shape,groups", rc.golden_shapes(), ids=lambda v: cases.case_id(v) if isinstance(v, tuple) else str(v))
def test_switch_off_describes_and_sizes_as_before(shape, groups):
    desc, nbytes = rc.load_golden()[(shape, groups)]
    assert desc.startswith("kind=dw_bf16 " if groups != 1 else "kind=bf16x1 ")
    assert rc.describe(shape, groups) == desc
    assert rc.workspace_bytes(shape, groups) == nbytes


def test_describe_shapes_of_the_existing_test_stay_on_the_tile_kernel():
    assert _lib.describe_bf16(2, 16, 10, 10, 16, 3, 3, 1, 1).startswith("kind=bf16x1 ")
    assert _lib.describe_bf16(256, 16, 224, 224, 16, 3, 3, 1, 1).startswith("kind=bf16x1 ")


# ---- switch on ----------------------------------------------------------------------------------------
def _plans():
    with _lib.bf16_rows():
        return [(s, rc.parse_rows(rc.describe(s))) for s in rc.TABLE]


def test_every_table_shape_runs_the_row_kernel():
    for s, p in _plans():
        N, C, H, W = s[:4]
        assert p.C == C and p.bands == -(-H // p.RB) and p.groups == -(-W // 16) and p.blocks == N * p.bands, (s, p)
        assert p.ring >= 2 and 0 < p.lds <= 64 * 1024, (s, p)
    with _lib.bf16_rows():
        for s in rc.TABLE:  # the pack is 3 tap rows x k-steps x nt fragments of 1 KiB behind the max|w| partials
            C = s[1]
            assert rc.workspace_bytes(s) == 1024 + 3 * (2 if C == 16 else 3) * (C // 16) * 1024, s
            assert rc.workspace_bytes(s, mode=0) == rc.workspace_bytes(s)


@pytest.mark.parametrize("shape,groups,what", rc.INELIGIBLE, ids=[w for _, _, w in rc.INELIGIBLE])
def test_ineligible_neighbours_keep_their_kernel(shape, groups, what):
    desc, nbytes = rc.load_golden()[(shape, groups)]
    with _lib.bf16_rows():
        assert rc.describe(shape, groups) == desc, what
        assert rc.workspace_bytes(shape, groups) == nbytes, what


def test_wmax_is_the_boundary_and_covers_both_flagship_widths():
    assert rc.WMAX >= 224
    with _lib.bf16_rows():
        for C in (16, 32):
            assert rc.describe(rc._c(1, C, 3, rc.WMAX)).startswith("kind=bf16_rows ")
            assert rc.describe(rc._c(1, C, 3, rc.WMAX + 2)).startswith("kind=bf16x1 ")
        assert rc.parse_rows(rc.describe(rc._c(256, 16, 224, 224))).RB == 16
        assert rc.parse_rows(rc.describe(rc._c(256, 32, 112, 112))).RB == 16


def _gpw(p):
    """Groups per wave of the instance: 1, 2 or 4."""
    g = -(-p.groups // rc.WAVES)
    return 1 if g <= 1 else (2 if g <= 2 else 4)


CONDITIONS = {  # name -> predicate of (shape, parsed description)
    "C = 16": lambda s, p: p.C == 16,
    "C = 32": lambda s, p: p.C == 32,
    "H = 1": lambda s, p: s[2] == 1,
    "H = 2": lambda s, p: s[2] == 2,
    "H = RB k (no ragged band)": lambda s, p: s[2] % p.RB == 0,
    "H = RB k + 1 (a one-row last band)": lambda s, p: s[2] > p.RB and s[2] % p.RB == 1,
    "more than one band per image": lambda s, p: p.bands > 1,
    "W = 2 (a single masked group)": lambda s, p: s[3] == 2 and p.groups == 1,
    "W = 16 g (no ragged group)": lambda s, p: s[3] % 16 == 0,
    "W = 16 g + 2 (a ragged last group)": lambda s, p: s[3] > 16 and s[3] % 16 == 2,
    "groups split unevenly over the waves": lambda s, p: p.groups > rc.WAVES and p.groups % rc.WAVES != 0,
    "an idle wave": lambda s, p: p.groups <= (rc.WAVES - 1) * _gpw(p),
    "W = Wmax with H = 3": lambda s, p: s[3] == rc.WMAX and s[2] == 3,
    "N = 3 with more than one band": lambda s, p: s[0] == 3 and p.bands > 1,
    "RB = 4": lambda s, p: p.RB == 4,
    "RB = 8": lambda s, p: p.RB == 8,
    "RB = 16": lambda s, p: p.RB == 16,
}
CONDITIONS.update({"C = %d with %d group(s) per wave" % (c, g): (lambda s, p, c=c, g=g: p.C == c and _gpw(p) == g)
                   for c in (16, 32) for g in (1, 2, 4)})


def test_case_table_meets_every_named_condition():
    plans = _plans()
    for name, cond in CONDITIONS.items():
        print("%s: %s" % (name, [cases.case_id(s) for s, p in plans if cond(s, p)]))
    unmet = [name for name, cond in CONDITIONS.items() if not any(cond(s, p) for s, p in plans)]
    assert not unmet, "no table shape meets: %s" % unmet
    assert sum(s[0] >= 2 for s in rc.TABLE) > len(rc.TABLE) // 2  # N >= 2 in most rows


# ---- the layers above the C ABI -------------------------------------------------------------------------
def test_meta_kernel_of_the_batched_pack_follows_the_switch():
    _lib.ops()
    elig, tile = rc._c(2, 32, 9, 16), (2, 16, 9, 18, 32, 3, 3, 1, 1, 1, 1, 1, 1)
    ws = [torch.empty(s[4], s[1], 3, 3, dtype=torch.bfloat16, device="meta") for s in (elig, tile)]
    geom = []
    for s in (elig, tile):
        geom += list(s[:4]) + list(s[7:13]) + [1]  # N, C, H, W, strides, pads, dilations, groups

    def sizes():
        out = torch.ops.po2q.qconv2d_pack_batch_bf16(ws, geom, [4, 4], [1, 1], [1, 1])
        return [int(t.numel()) for t in out]

    off = sizes()
    assert off == [rc.workspace_bytes(elig), rc.workspace_bytes(tile)]
    with _lib.bf16_rows():
        on = sizes()
        assert on == [rc.workspace_bytes(elig), rc.workspace_bytes(tile)]
    assert on[0] != off[0] and on[1] == off[1]


def test_ptq_row_kernel_option():
    ap = ptq.arg_parser()
    base = ["resnet20", "cifar", "--data_file", "x.pt"]
    assert ap.parse_args(base).bf16_row_kernels is False
    assert ap.parse_args(base + ["--dtype", "bf16", "--bf16-row-kernels"]).bf16_row_kernels is True
    with pytest.raises(AssertionError, match="--bf16-row-kernels needs --dtype bf16"):
        ptq.main("resnet20", "cifar", "x.pt", bf16_row_kernels=True)
