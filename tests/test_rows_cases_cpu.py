"""Host proof for tests/_rows_cases.py (no GPU): the table's rows reach every instance of the four row-streaming
kernels that the planners, the *_res_ok predicates and the env switches can produce, each row's selector finds its
plan, and each named geometry condition holds -- all from `_lib.plans` descriptions and the shapes alone."""
import collections
import itertools

import pytest

from tests import _rows_cases as R

LAUNCHABLE = R.launchable()

# Launchable instances no planner reaches, with the rule that forbids each (all conv_rows2 with the fused shortcut,
# which only po2q_qconv2d_s2ds_f32 launches, on the plan s2ds_plan picks):
#   NTS = 1: s2ds_plan skips every candidate with nts != 0;
#   C = 16, PD = 2: s2ds_plan prefers ring depth 4, and rows2_candidates always offers it -- the depth-4 plan of the
#   widest row (7 waves, W = 224) takes 92,480 + 2,048 bytes of the 163,840.
UNPRODUCIBLE = {("rows2", 16, pd, e, n, nd, 1) for pd in (2, 4) for e in (0, 1) for n in (0, 1) for nd in (1, 2)
                if n == 1 or pd == 2}
PRODUCIBLE = LAUNCHABLE - UNPRODUCIBLE

SWEEP_W = (4, 8, 16, 20, 24, 32, 36, 40, 64, 100, 112, 116, 196, 224, 228)
SWEEP = [(N, C, H, W, K, st)
         for C, K, st in ((16, 16, 1), (32, 16, 1), (32, 32, 1), (64, 64, 1), (16, 32, 2), (32, 64, 2))
         for N in (1, 2, 3, 9) for H in (3, 4, 5, 6, 7, 8, 9, 13, 17, 33) for W in SWEEP_W]


def _all_keys(shape, i, p, picks):
    """Every instance key candidate i (plan p) of `shape` can run as: call forms x PIPE settings x RES switch."""
    forms = ["plain", "epi", "res"]
    if p.vr == 5 and picks.get(shape) is not None and picks[shape][0] == i:
        forms += ["ds", "ds_epi"]
    for f in forms:
        for pipe in ((None, 0, 1) if shape[1] == 64 else (None,)):
            for res_on in ((True, False) if f == "res" and shape[1] == 64 else (True,)):
                yield f, pipe, res_on, R.dispatch(p, shape, f, pipe, res_on)


@pytest.fixture(scope="module")
def sweep():
    """instance key -> one (shape, description) that reaches it, over SWEEP; and the refused candidates."""
    reach, refused = {}, []
    for shape in SWEEP:
        descs = R.plans(shape)
        picks = {shape: R.s2ds_pick(shape)} if shape[5] == 2 else {}
        for i, d in enumerate(descs):
            if "kind=bf16x3_rows" not in d:
                continue
            p = R.parse(d)
            for f, pipe, res_on, k in _all_keys(shape, i, p, picks):
                if k is None or k not in LAUNCHABLE:
                    refused.append((shape, d, f, pipe, res_on, k))
                else:
                    reach.setdefault(k, (shape, d))
    return reach, refused


def test_launchable_set_size():
    n = collections.Counter(k[0] for k in LAUNCHABLE)
    assert n == {"rows": 20, "rowsf": 156, "rowsk": 66, "rows2": 48} and len(LAUNCHABLE) == 290
    assert UNPRODUCIBLE <= LAUNCHABLE and len(UNPRODUCIBLE) == 12 and len(PRODUCIBLE) == 278


def test_every_offered_candidate_is_launchable(sweep):
    """A candidate the dispatch would refuse with hipErrorInvalidValue is a bug."""
    assert not sweep[1], sweep[1][:5]


def test_planners_offer_exactly_the_producible_set(sweep):
    reach = sweep[0]
    assert not (set(reach) & UNPRODUCIBLE), sorted(set(reach) & UNPRODUCIBLE)
    assert not (PRODUCIBLE - set(reach)), sorted(PRODUCIBLE - set(reach))


def test_rowsf_residual_ring_always_fits():
    """rowsf_res_ok's LDS bound never turns false: the largest ring of any full-row plan (C = 32, 7 waves, 4 slots)
    is 157,984 bytes of the 163,840, so no full-row plan leaves its residual to the elementwise pass.  (The pass is
    covered on the plans of conv_rows, conv_rows2 and conv_rowsk's C = 32 MFMA-wave variants: `res_by_pass`.)"""
    worst = max(R.rowsf_res_lds(C, nw, pd) for C, pds in ((16, (3, 4)), (32, (2, 3, 4))) for nw in range(1, 8) for pd in pds)
    assert worst == R.rowsf_res_lds(32, 7, 4) == 157984 <= R.LDS_CU


def _found():
    out = []
    for r in R.ROWS:
        f = R.find_plan(r)
        assert f is not None, "plan not found: " + R.row_id(r)
        assert R.find_plan(r, "po2+") is not None, "plan not found in po2+: " + R.row_id(r)
        out.append((r, f[1]))
    return out


def _coverage(found):
    """instance key -> rows, condition -> rows."""
    inst, cond = collections.defaultdict(list), collections.defaultdict(list)
    for n, (r, p) in enumerate(found):
        for k in set(R.row_keys(r, p).values()):
            inst[k].append(n)
        for c in r.conds:
            cond[c].append(n)
    return inst, cond


def test_rows_reach_every_producible_instance():
    found = _found()
    inst, _ = _coverage(found)
    for r, p in found:
        for fk, k in R.row_keys(r, p).items():
            assert k in PRODUCIBLE, (R.row_id(r), fk, k)
    missing = sorted(PRODUCIBLE - set(inst))
    assert not missing, "instances without a case: %s" % missing


def test_named_conditions_hold_and_are_all_covered():
    found = _found()
    _, cond = _coverage(found)
    for r, p in found:
        for c in r.conds:
            ok = R.CONDS[c](p, r.shape) if c in R.CONDS else R.RUN_CONDS[c](r, p)
            assert ok, "%s does not meet its condition %s (%s)" % (R.row_id(r), c, p)
    missing = sorted((set(R.CONDS) | set(R.RUN_CONDS)) - set(cond))
    assert not missing, "conditions without a case: %s" % missing


def test_every_row_is_needed():
    """Each row is the only case of some instance or condition: removing any one fails one of the two tests above."""
    found = _found()
    inst, cond = _coverage(found)
    for n, (r, p) in enumerate(found):
        only = [k for k, rows in itertools.chain(inst.items(), cond.items()) if rows == [n]]
        assert only, "redundant row: " + R.row_id(r)


def test_rows_are_small():
    for r in R.ROWS:
        N, C, H, W, K, st = r.shape
        assert N <= 4 and H <= 17 and W <= 228, r.shape
        assert W <= 40 or any(c in r.conds for c in ("f16_7waves", "f32_7waves", "f_last_strip_4", "f_res_ring_max",
                                                     "s_7waves")) or r.sel["vr"] == 0, r.shape


def test_bitwise_siblings_exist():
    for r in R.ROWS:
        for sel in R.siblings(r):
            for mode in ("po2", "po2+"):
                assert R.find_plan(r, mode, sel) is not None, (R.row_id(r), sel)


def test_s2ds_rows_are_the_plan_the_fused_transition_runs():
    for r in R.ROWS:
        if "ds" in r.forms:
            for mode in ("po2", "po2+"):
                assert R.s2ds_pick(r.shape, mode)[0] == R.find_plan(r, mode)[0], R.row_id(r)


def test_too_short_shapes_get_no_row_plan():
    for shape, absent in R.FALLBACK_SHAPES:
        vrs = {R.parse(d).vr for d in R.plans(shape) if "kind=bf16x3_rows" in d}
        assert not (vrs & set(absent)), (shape, vrs)


def test_instances_the_earlier_conv_shapes_reached():
    """The gap this table closes: tests/test_gpu_conv.py's every-candidate test over its 3x3 SHAPES runs the plain
    form only, its fused tests add epilogue / residual forms on six shapes -- together 173 of the 278 producible
    instances when this table was added (none under PO2Q_ROWSK_PIPE = 0 / 1, none of the fused-shortcut ones, few residual ones)."""
    shapes = [(2, 16, 40, 36, 16, 1), (2, 32, 20, 20, 32, 1), (1, 64, 14, 14, 64, 1), (2, 16, 33, 31, 32, 2),
              (2, 32, 16, 16, 64, 2), (3, 16, 8, 8, 16, 1), (2, 16, 5, 4, 16, 1), (1, 16, 37, 68, 16, 1),
              (1, 32, 23, 20, 16, 1), (2, 32, 1, 12, 32, 1), (2, 16, 1, 36, 16, 1), (1, 16, 9, 220, 16, 1),
              (2, 64, 12, 40, 64, 1), (1, 64, 3, 8, 64, 1), (2, 16, 40, 40, 32, 2), (1, 16, 9, 64, 32, 2),
              (1, 16, 17, 8, 32, 2), (2, 16, 30, 224, 32, 2), (2, 32, 40, 40, 64, 2), (1, 32, 17, 8, 64, 2),
              (2, 32, 30, 112, 64, 2)]
    fused = {(2, 16, 20, 32, 16, 1): ("epi", "res"), (1, 32, 13, 36, 32, 1): ("epi", "res"),
             (1, 64, 9, 40, 64, 1): ("epi", "res"), (2, 64, 5, 56, 64, 1): ("res",), (1, 64, 6, 40, 64, 1): ("res",),
             (3, 64, 7, 8, 64, 1): ("res",), (1, 64, 12, 36, 64, 1): ("res",), (2, 16, 40, 36, 16, 1): ("epi", "res"),
             (2, 32, 20, 24, 32, 1): ("epi", "res"), (1, 64, 12, 40, 64, 1): ("epi", "res"),
             (2, 16, 40, 40, 32, 2): ("epi", "res")}
    got = set()
    for shape in shapes:
        for d in R.plans(shape, "po2+"):
            if "kind=bf16x3_rows" in d:
                got.add(R.dispatch(R.parse(d), shape, "plain"))
    for shape, forms in fused.items():
        descs = R.plans(shape)
        every = shape in ((2, 16, 20, 32, 16, 1), (1, 32, 13, 36, 32, 1), (1, 64, 9, 40, 64, 1)) or forms == ("res",)
        for d in (descs if every else descs[:1]):
            if "kind=bf16x3_rows" in d:
                got |= {R.dispatch(R.parse(d), shape, f) for f in forms}
    got.discard(None)
    print("instances reached by test_gpu_conv.py's shapes: %d of %d" % (len(got & PRODUCIBLE), len(PRODUCIBLE)))
    assert len(got & PRODUCIBLE) < len(PRODUCIBLE)
