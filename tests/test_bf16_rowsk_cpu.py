"""Host side of the C = K = 64 bf16 row-streaming conv kernel (conv_b16_rowsk, "kind=bf16_rowsk"): its own
opt-in switch and that switch's independence of the first row kernel's, the planner with the switch off
and on, the eligibility boundary and the case table's coverage.  Needs the built library, no device.

With the new switch off nothing may differ from the library before the kernel existed, whatever the first
switch says: the golden list of tests/_bf16_rows_cases.py (written by the library before either row
kernel) still holds, and every shape of both tables plans as in a run with both switches off."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from po2_quantization_amd import _lib, ptq
from po2_quantization_amd.models import quantized_conv
from tests import _bf16_rows_cases as rc
from tests import _bf16_rowsk_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def both_switches_off_around_each_test():
    prev = _lib.set_bf16_row_kernels(False), _lib.set_bf16_rowsk_kernels(False)
    yield
    _lib.set_bf16_row_kernels(prev[0])
    _lib.set_bf16_rowsk_kernels(prev[1])


def plan_of(shape, groups=1):
    return kc.describe(shape, groups), kc.workspace_bytes(shape, groups), kc.workspace_bytes(shape, groups, mode=0)


# ---- the switch ------------------------------------------------------------------------------------
def test_symbols_exported():
    L = _lib.load()
    for name in ("po2q_bf16_set_rowsk_kernels", "po2q_bf16_rowsk_kernels"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "po2q.h")) as f:
        header = f.read()
    assert "int po2q_bf16_set_rowsk_kernels(int on);" in header and "int po2q_bf16_rowsk_kernels(void);" in header


def _child(env, code):
    full = dict(os.environ)
    for name in ("PO2Q_B16_ROWS", "PO2Q_B16_ROWSK"):
        full.pop(name, None)
    full.update(env)
    full["PYTHONPATH"] = ROOT + os.pathsep + full.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", code], env=full, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.strip()


def test_switch_defaults_to_off_and_follows_its_own_environment_variable_in_a_fresh_process():
    code = ("from po2_quantization_amd import _lib\n"
            "print(int(_lib.bf16_row_kernels()), int(_lib.bf16_rowsk_kernels()),"
            " _lib.describe_bf16(2, 64, 9, 18, 64, 3, 3, 1, 1).split()[0],"
            " _lib.describe_bf16(2, 16, 9, 18, 16, 3, 3, 1, 1).split()[0])")
    assert _child({}, code) == "0 0 kind=bf16x1 kind=bf16x1"
    assert _child({"PO2Q_B16_ROWSK": "0"}, code) == "0 0 kind=bf16x1 kind=bf16x1"
    assert _child({"PO2Q_B16_ROWSK": "1"}, code) == "0 1 kind=bf16_rowsk kind=bf16x1"
    assert _child({"PO2Q_B16_ROWS": "1"}, code) == "1 0 kind=bf16x1 kind=bf16_rows"
    assert _child({"PO2Q_B16_ROWS": "1", "PO2Q_B16_ROWSK": "1"}, code) == "1 1 kind=bf16_rowsk kind=bf16_rows"


def test_setter_returns_the_previous_value():
    assert _lib.bf16_rowsk_kernels() is False
    assert _lib.set_bf16_rowsk_kernels(True) is False
    assert _lib.bf16_rowsk_kernels() is True
    assert _lib.set_bf16_rowsk_kernels(True) is True
    assert _lib.set_bf16_rowsk_kernels(False) is True
    assert _lib.bf16_rowsk_kernels() is False
    L = _lib.load()
    assert L.po2q_bf16_set_rowsk_kernels(7) == 0 and L.po2q_bf16_rowsk_kernels() == 1  # any non-zero value: on
    assert L.po2q_bf16_set_rowsk_kernels(-1) == 1 and L.po2q_bf16_rowsk_kernels() == 1
    assert L.po2q_bf16_set_rowsk_kernels(0) == 1 and L.po2q_bf16_rowsk_kernels() == 0


def test_context_manager_restores_the_previous_value():
    with _lib.bf16_rowsk():
        assert _lib.bf16_rowsk_kernels()
        with _lib.bf16_rowsk(False):
            assert not _lib.bf16_rowsk_kernels()
        assert _lib.bf16_rowsk_kernels()
    assert not _lib.bf16_rowsk_kernels()
    with pytest.raises(ZeroDivisionError):
        with _lib.bf16_rowsk():
            1 / 0
    assert not _lib.bf16_rowsk_kernels()


def test_the_two_switches_do_not_touch_each_other():
    for first in (False, True):
        _lib.set_bf16_row_kernels(first)
        for new in (True, False, True):
            _lib.set_bf16_rowsk_kernels(new)
            assert _lib.bf16_row_kernels() is first and _lib.bf16_rowsk_kernels() is new
    for new in (False, True):
        _lib.set_bf16_rowsk_kernels(new)
        for first in (True, False, True):
            _lib.set_bf16_row_kernels(first)
            assert _lib.bf16_row_kernels() is first and _lib.bf16_rowsk_kernels() is new
        with _lib.bf16_rows(not _lib.bf16_row_kernels()):
            assert _lib.bf16_rowsk_kernels() is new
        assert _lib.bf16_rowsk_kernels() is new


def first_eligible(shape, groups):
    """The first switch's eligibility as include/po2q.h states it."""
    N, C, H, W, K = shape[:5]
    return (groups == 1 and tuple(shape[5:]) == (3, 3, 1, 1, 1, 1, 1, 1) and C == K and C in (16, 32)
            and W % 2 == 0 and W <= rc.WMAX)


# ---- new switch off: the parent's planner, byte for byte, under either setting of the first switch ------
def test_new_switch_off_plans_as_before_under_either_setting_of_the_first_switch():
    golden = rc.load_golden()
    assert all(first_eligible(s, 1) for s in rc.TABLE)
    for shape, groups in kc.all_shapes():
        both_off = plan_of(shape, groups)
        if (shape, groups) in golden:
            assert both_off[:2] == golden[(shape, groups)], (shape, groups)
        assert not both_off[0].startswith("kind=bf16_rows"), both_off
        with _lib.bf16_rows():
            first_on = plan_of(shape, groups)
        if first_eligible(shape, groups):  # what tests/test_bf16_rows_cpu.py pins for the first switch
            assert first_on[0].startswith("kind=bf16_rows "), (shape, first_on)
            assert first_on[1] == 1024 + 3 * (2 if shape[1] == 16 else 3) * (shape[1] // 16) * 1024
        else:
            assert first_on == both_off, (shape, groups)


def test_every_table_shape_is_on_the_tile_kernel_with_the_new_switch_off():
    for first in (False, True):
        with _lib.bf16_rows(first):
            for s in kc.TABLE:
                assert kc.describe(s).startswith("kind=bf16x1 "), (s, first)


# ---- new switch on ------------------------------------------------------------------------------------
def _plans():
    with _lib.bf16_rowsk():
        return [(s, kc.parse_rowsk(kc.describe(s))) for s in kc.TABLE]


def test_every_table_shape_runs_the_new_kernel():
    for s, p in _plans():
        N, C, H, W = s[:4]
        assert p.C == C == 64 and p.bands == -(-H // p.RB) and p.groups == -(-W // 16), (s, p)
        assert p.blocks == N * p.bands and p.GW in (1, 2, 4) and p.GW // 2 < p.groups <= p.GW, (s, p)
        # two planes [W + 2][64] bf16 and four wave tiles [16][16 GW] bf16 with a 16-byte pitch pad
        assert p.ring == 2 and p.lds == 2 * (W + 2) * 128 + 4 * 16 * (32 * p.GW + 16) <= 64 * 1024, (s, p)
    frag_bytes = 4 * 3 * 6 * 64 * 16  # [channel tile][tap row][k-step][lane][8] bf16
    for first in (False, True):
        with _lib.bf16_rows(first), _lib.bf16_rowsk():
            for s in kc.TABLE:
                assert kc.workspace_bytes(s) == 1024 + frag_bytes, s  # behind the max|w| partials
                assert kc.workspace_bytes(s) > 0 and kc.workspace_bytes(s) >= frag_bytes
                assert kc.workspace_bytes(s, mode=0) == kc.workspace_bytes(s)
                assert kc.is_rowsk(s)


@pytest.mark.parametrize("shape,groups,what", kc.INELIGIBLE, ids=[w for _, _, w in kc.INELIGIBLE])
def test_ineligible_neighbours_keep_their_plan(shape, groups, what):
    both_off = plan_of(shape, groups)
    assert not both_off[0].startswith("kind=bf16_rows"), what
    with _lib.bf16_rowsk():
        assert plan_of(shape, groups) == both_off, what


def test_only_the_newly_eligible_layers_change_with_the_new_switch_on():
    eligible = set(kc.TABLE) | {rc._c(2, 64, 9, 18)}
    for first in (False, True):
        with _lib.bf16_rows(first):
            for shape, groups in kc.all_shapes():
                off = plan_of(shape, groups)
                with _lib.bf16_rowsk():
                    on = plan_of(shape, groups)
                if shape in eligible and groups == 1:
                    assert on[0].startswith("kind=bf16_rowsk ") and on != off, (shape, first)
                else:
                    assert on == off, (shape, groups, first)


def test_wmax_is_the_boundary_and_covers_the_flagship_width():
    assert kc.WMAX >= 56
    with _lib.bf16_rowsk():
        assert kc.is_rowsk(kc._c(1, 64, 3, kc.WMAX))
        assert kc.describe(kc._c(1, 64, 3, kc.WMAX + 2)).startswith("kind=bf16x1 ")
        p = kc.parse_rowsk(kc.describe(kc._c(256, 64, 56, 56)))
        assert (p.RB, p.bands, p.groups, p.GW, p.blocks) == (16, 4, 4, 4, 1024)


CONDITIONS = {  # name -> predicate of (shape, parsed description)
    "GW = 1": lambda s, p: p.GW == 1,
    "GW = 2": lambda s, p: p.GW == 2,
    "GW = 4": lambda s, p: p.GW == 4,
    "GW = 4 with an idle group slot": lambda s, p: p.GW == 4 and p.groups == 3,
    "RB = 4": lambda s, p: p.RB == 4,
    "RB = 8": lambda s, p: p.RB == 8,
    "RB = 16": lambda s, p: p.RB == 16,
    "a ragged last band": lambda s, p: p.bands > 1 and s[2] % p.RB != 0,
    "RB = 16 with a one-row last band": lambda s, p: p.RB == 16 and s[2] > 16 and s[2] % 16 == 1,
    "more than one band per image": lambda s, p: p.bands > 1,
    "a ragged last group behind a full one": lambda s, p: p.groups > 1 and s[3] % 16 != 0,
    "a half-filled single group": lambda s, p: p.groups == 1 and s[3] == 8,
    "one exactly full group": lambda s, p: s[3] == 16,
    "H = 1": lambda s, p: s[2] == 1,
    "H = 2": lambda s, p: s[2] == 2,
    "W = 2": lambda s, p: s[3] == 2,
    "W = Wmax, every group full": lambda s, p: s[3] == kc.WMAX and p.groups == 4,
    "W = 56 (ResNet56 @224, stage 3)": lambda s, p: s[3] == 56,
    "N = 3": lambda s, p: s[0] == 3,
    "N >= 2 with more than one band": lambda s, p: s[0] >= 2 and p.bands > 1,
}


def test_case_table_meets_every_named_condition():
    plans = _plans()
    for name, cond in CONDITIONS.items():
        print("%s: %s" % (name, [kc.case_id(s) for s, p in plans if cond(s, p)]))
    unmet = [name for name, cond in CONDITIONS.items() if not any(cond(s, p) for s, p in plans)]
    assert not unmet, "no table shape meets: %s" % unmet


# ---- the layers above the C ABI -------------------------------------------------------------------------
def test_meta_kernel_of_the_batched_pack_follows_the_new_switch():
    _lib.ops()
    shapes = (kc._c(2, 64, 9, 18), rc._c(2, 32, 9, 16), (2, 64, 9, 18, 128, 3, 3, 1, 1, 1, 1, 1, 1))
    ws = [torch.empty(s[4], s[1], 3, 3, dtype=torch.bfloat16, device="meta") for s in shapes]
    geom = []
    for s in shapes:
        geom += list(s[:4]) + list(s[7:13]) + [1]  # N, C, H, W, strides, pads, dilations, groups

    def sizes():
        out = torch.ops.po2q.qconv2d_pack_batch_bf16(ws, geom, [4] * 3, [1] * 3, [1] * 3)
        got = [int(t.numel()) for t in out]
        assert got == [kc.workspace_bytes(s) for s in shapes]
        return got

    off = sizes()
    with _lib.bf16_rowsk():
        on = sizes()
        with _lib.bf16_rows():
            both = sizes()
    assert on[0] == 1024 + 4 * 18 * 1024 and on[0] != off[0] and on[1:] == off[1:]
    assert both[0] == on[0] and both[1] != on[1] and both[2] == on[2]


def test_ptq_rowsk_kernel_option():
    ap = ptq.arg_parser()
    base = ["resnet20", "cifar", "--data_file", "x.pt"]
    assert ap.parse_args(base).bf16_rowsk_kernels is False
    a = ap.parse_args(base + ["--dtype", "bf16", "--bf16-rowsk-kernels"])
    assert a.bf16_rowsk_kernels is True and a.bf16_row_kernels is False
    a = ap.parse_args(base + ["--dtype", "bf16", "--bf16-row-kernels"])
    assert a.bf16_rowsk_kernels is False and a.bf16_row_kernels is True
    with pytest.raises(AssertionError, match="--bf16-rowsk-kernels needs --dtype bf16"):
        ptq.main("resnet20", "cifar", "x.pt", bf16_rowsk_kernels=True)
    assert not _lib.bf16_rowsk_kernels()


def test_ptq_puts_the_setting_back(monkeypatch, tmp_path):
    """main() sets the switch for the run and restores it: the device check and the seed walk are stubbed,
    the evaluation sees the requested setting."""
    seen = []
    monkeypatch.setattr(ptq.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ptq, "init", lambda: None)
    monkeypatch.setattr(ptq, "tensor_loader", lambda *a: [])
    monkeypatch.setattr(ptq.glob, "glob", lambda pat: ["seed0"])
    monkeypatch.setattr(ptq, "write_results", lambda *a: None)
    monkeypatch.setattr(ptq, "evaluate_seed",
                        lambda *a, **k: seen.append((_lib.bf16_row_kernels(), _lib.bf16_rowsk_kernels())))
    for prev in (False, True):
        _lib.set_bf16_rowsk_kernels(prev)
        for want in (True, False):
            ptq.main("resnet20", "cifar", "x.pt", train_dir=str(tmp_path), results_dir=str(tmp_path / "r"),
                     dtype="bf16", bf16_rowsk_kernels=want)
            assert seen[-1] == (False, want)
            assert _lib.bf16_rowsk_kernels() is prev and _lib.bf16_row_kernels() is False


def test_pack_record_key_carries_both_switches():
    model = nn.Sequential(quantized_conv.QuantizedConv2d(64, 64, 3))
    keys = {}
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.zeros(1, 64, 8, 8, dtype=dtype)
        for first in (False, True):
            for new in (False, True):
                with _lib.bf16_rows(first), _lib.bf16_rowsk(new):
                    keys[(dtype, first, new)] = quantized_conv._record_key(model, x)
                    assert quantized_conv._record_key(model, x) == keys[(dtype, first, new)]
    assert len(set(keys.values())) == len(keys) == 8
