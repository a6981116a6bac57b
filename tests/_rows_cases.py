"""Case table and helpers shared by tests/test_rows_cases_cpu.py and tests/test_gpu_rows_paths.py.

The four row-streaming kernels behind kind bf16x3_rows of the fp32 entry -- conv_rows (po2q_conv_rows.hip, plan
vr 0), conv_rowsf (po2q_conv_rowsf.hip, vr 4), conv_rowsk (po2q_conv_rowsk.hip, vr 1 / 2 / 3) and conv_rows2
(po2q_conv_rows2.hip, vr 5) -- are templates with some 290 launchable instances.  Which instance runs depends on the
candidate plan (the planners keep the cheapest two or three segment heights of a shape, and the candidate list the
cheapest 40 row plans), on the call form (plain, affine / activation epilogue, residual), on the *_res_ok predicates
and on the PO2Q_ROWSK_PIPE / PO2Q_ROWSK_RES switches.

`dispatch` restates the launch macros: (plan description, shape, call form, switches) -> instance key.  Every row
of ROWS is (shape, plan selector, call forms, PIPE settings, named geometry conditions); the selector matches
fields of the plan description, never a candidate index.  The CPU test proves that the rows reach every instance
the planners can produce and that each named condition holds; the GPU test runs every row against the oracle.

Shapes are (N, C, H, W, K, stride): 3x3, pad 1, dilation 1, groups 1 throughout."""
import collections
import re

from po2_quantization_amd import _lib
from tests import _tile_cases as T

KIB = 1024
LDS_CU = 160 * KIB

Plan = collections.namedtuple("Plan", "kind CC NT NJ vr TP TQ tilesP tilesQ lds blocks pd nts var fp")
_PLAN_RE = re.compile(
    r"kind=(\S+) CC=(\d+) NT=(\d+) MI=\d+ NJ=(\d+) vr=(\d+) tile=(\d+)x(\d+) tiles=(\d+)x(\d+) halo=\d+x\d+ "
    r"chunks=\d+ kblocks=\d+ ksteps=\d+ lds=(\d+) blocks=(\d+) waves=\d+ ov=\d+ wstream=\d+ pd=(\d+) nts=(\d+) "
    r"var=(\d+) fp=(\d+)$")


def parse(desc):
    m = _PLAN_RE.match(desc)
    assert m, "not a plan description: %r" % desc
    g = m.groups()
    return Plan(g[0], *map(int, g[1:]))


def shape13(shape):
    N, C, H, W, K, st = shape
    return (N, C, H, W, K, 3, 3, st, st, 1, 1, 1, 1)


def out_size(shape):
    return T.out_size(shape13(shape))


def plans(shape, mode="po2"):
    return T.plans(shape13(shape), None, mode)


# ---- the kernels' geometry, restated (description + shape only) --------------------------------------------------
def waves(p, shape):
    """Waves per block of a full-row plan (vr 4: strips of 512 / C columns; vr 5: strips of 16 output columns)."""
    if p.vr == 4:
        return p.TQ // (512 // shape[1])
    if p.vr == 5:
        return p.TQ // 16
    raise AssertionError(p)


def strip(p, shape):
    """Output columns per strip: a wave's strip of the full-row kernels, a work item's of conv_rows / conv_rowsk."""
    if p.vr == 4:
        return 512 // shape[1]
    if p.vr == 5:
        return 16
    return p.TQ


def items(p, shape):
    return shape[0] * p.tilesP * p.tilesQ


def last_segment(p, shape):
    P, _ = out_size(shape)
    return P - (p.tilesP - 1) * p.TP


def last_strip(p, shape):
    _, Q = out_size(shape)
    s = strip(p, shape)
    return Q - ((Q - 1) // s) * s


def rows2_nd(p, shape):
    """conv_rows2's DMA count per wave and input row (rows2_candidates: float4s of a row over the block's lanes)."""
    return -(-(shape[1] * shape[3] // 4) // (64 * waves(p, shape)))


def rowsf_lds(C, nwaves, pd):
    """rowsf_lds (po2q_conv_rowsf.hip): B fragments + raw ring + three bf16 planes per wave."""
    sw = 512 // C
    plane = (sw + 2) * C * 2 + 32
    wbytes = 3 * (2 if C == 16 else 3) * (C // 16) * 1024
    return wbytes + pd * C * sw * nwaves * 4 + nwaves * 3 * plane


def rowsf_res_lds(C, nwaves, pd):
    """rowsf_res_lds: + one 2 KiB residual slot per wave and ring slot."""
    return rowsf_lds(C, nwaves, pd) + nwaves * pd * 2048


# ---- the launch dispatch, restated ----------------------------------------------------------------------------------
FORMS = ("plain", "epi", "res", "ds", "ds_epi")
ROWS_CFG = ((16, 1, 2), (16, 1, 3), (16, 1, 6), (32, 1, 2), (32, 2, 2))             # PO2Q_ROWS_NTS: (CC, NT, PD)
RF16_NV = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (3, 0), (3, 1))                   # PO2Q_RF16 / PO2Q_RFR: (NTS, V)
RF32_NV = ((0, 0), (0, 1), (2, 0), (2, 1))


def launchable():
    """Every instance a launch_* can instantiate outside PO2Q_ROWS_DIAG, from the dispatch macros.
    conv_rows  (CC, NT, EPI, NTS, PD)                     rows_dispatch: PO2Q_ROWS_NTS
    conv_rowsf (CC, PD, EPI, NTS, V, RES, FP)             launch_conv_rowsf: PO2Q_RF; _res: PO2Q_RFR; launch_rowsf_t: FP
    conv_rowsk (C, PD, TT, LW, EPI, NTS, RES, FP, PIPE)   launch_conv_rowsk: PO2Q_RKF / RKP / RKPN / RK / RK1 / RKN;
                                                          _res: the two C = 64 launches and PO2Q_RKR
    conv_rows2 (CC, PD, EPI, NTS, ND, DS)                 launch_conv_rows2: PO2Q_R2; launch_rows2_t: ND; _nd: DS"""
    s = set()
    for cc, nt, pd in ROWS_CFG:
        s |= {("rows", cc, nt, e, n, pd) for e in (0, 1) for n in (0, 1)}
    for fp in (0, 1):
        for pd in (3, 4):
            for n, v in RF16_NV:
                s |= {("rowsf", 16, pd, e, n, v, 0, fp) for e in (0, 1)} | {("rowsf", 16, pd, 1, n, v, 1, fp)}
        for pd in (2, 3, 4):
            for n, v in RF32_NV:
                s |= {("rowsf", 32, pd, e, n, v, 0, fp) for e in (0, 1)} | {("rowsf", 32, pd, 1, n, v, 1, fp)}
    for e in (0, 1):
        for pd in (2, 3):
            s.add(("rowsk", 64, pd, 0, 0, e, 0, 0, 1, 0))                                 # PO2Q_RKF
            s |= {("rowsk", 64, pd, tt, 0, e, 0, 0, 0, 1) for tt in (0, 1)}               # PO2Q_RKP
            s |= {("rowsk", 64, pd, 0, 0, e, n, 0, 0, 1) for n in (1, 2, 3)}              # PO2Q_RKPN
            s |= {("rowsk", c, pd, tt, 0, e, 0, 0, 0, 0) for c in (32, 64) for tt in (0, 1)}  # PO2Q_RK
            s |= {("rowsk", 64, pd, 0, 0, e, n, 0, 0, 0) for n in (1, 2, 3)}              # PO2Q_RKN (C = 64)
        s |= {("rowsk", 32, 3, 1, 1, e, n, 0, 0, 0) for n in (0, 1, 2, 3)}                # PO2Q_RK1 / RKN (loader wave)
    s |= {("rowsk", 64, 2, 1, 0, 1, 0, 1, fp, 0) for fp in (0, 1)}                        # launch_conv_rowsk_res, C = 64
    s |= {("rowsk", 32, 3, 1, 1, 1, n, 1, 0, 0) for n in (0, 1, 2, 3)}                    # PO2Q_RKR
    for e in (0, 1):
        for ds in (0, 1):
            s |= {("rows2", 16, pd, e, n, nd, ds) for pd in (2, 4) for n in (0, 1) for nd in (1, 2)}
            s |= {("rows2", 32, 2, e, 0, nd, ds) for nd in (1, 2, 3, 4)}
    return s


def res_in_kernel(p, shape, res_on=True):
    """rows_res_ok: whether the residual add runs in the kernel's stores (else: an elementwise pass after it)."""
    N, C, H, W, K, st = shape
    if p.vr == 4:      # rowsf_res_ok: rowsf_plan_ok and the residual ring fits LDS
        nw = waves(p, shape)
        return (C, K) in ((16, 16), (32, 32)) and 1 <= nw <= 7 and rowsf_res_lds(C, nw, p.pd) <= LDS_CU
    if (C, K) == (32, 32):     # rowsk_res_ok
        return p.vr == 3 and p.pd == 3 and not p.fp
    return (C, K) == (64, 64) and p.vr in (1, 2) and res_on


def dispatch(p, shape, form, pipe=None, res_on=True):
    """The instance key the library launches for plan p of `shape` under call form `form` (run_plan in po2q_capi.hip,
    then the launch_* dispatch), or None where the dispatch returns hipErrorInvalidValue.
    pipe: PO2Q_ROWSK_PIPE (None: unset); res_on: PO2Q_ROWSK_RES is not 0."""
    N, C, H, W, K, st = shape
    assert p.kind == "bf16x3_rows" and form in FORMS
    if form in ("ds", "ds_epi"):       # po2q_qconv2d_s2ds_f32 -> launch_conv_rows2 with yds
        if p.vr != 5 or p.lds + (K // 16) * KIB > LDS_CU:
            return None
        ds, epi = 1, int(form == "ds_epi")
    else:
        ds = 0
        if form == "res" and res_in_kernel(p, shape, res_on):
            if p.vr == 4:              # launch_conv_rowsf_res
                nv = RF16_NV if C == 16 else RF32_NV
                pds = (3, 4) if C == 16 else (2, 3, 4)
                return ("rowsf", C, p.pd, 1, p.nts, p.var, 1, p.fp) if (p.nts, p.var) in nv and p.pd in pds else None
            if C == 64:                # launch_conv_rowsk_res: the TT sibling with two ring slots, whatever pd / nts
                return ("rowsk", 64, 2, 1, 0, 1, 0, 1, p.fp, 0)
            return ("rowsk", 32, 3, 1, 1, 1, p.nts, 1, 0, 0) if p.nts in (0, 1, 2, 3) else None
        epi = int(form != "plain")     # a residual the kernel cannot add: affine in the kernel, then a pass
    if p.vr == 5:                      # launch_conv_rows2
        if not p.fp or p.var or (C, K) not in ((16, 32), (32, 64)):
            return None
        nd = rows2_nd(p, shape)
        if C == 16:
            ok = p.pd in (2, 4) and p.nts in (0, 1) and nd in (1, 2)
        else:
            ok = p.pd == 2 and p.nts == 0 and nd in (1, 2, 3, 4)
        return ("rows2", C, p.pd, epi, p.nts, nd, ds) if ok else None
    if p.vr == 4:                      # launch_conv_rowsf
        nw = waves(p, shape)
        if (C, K) not in ((16, 16), (32, 32)) or not 1 <= nw <= 7 or p.TQ != nw * (512 // C):
            return None
        nv = RF16_NV if C == 16 else RF32_NV
        pds = (3, 4) if C == 16 else (2, 3, 4)
        return ("rowsf", C, p.pd, epi, p.nts, p.var, 0, p.fp) if (p.nts, p.var) in nv and p.pd in pds else None
    if p.vr in (1, 2, 3):              # launch_conv_rowsk
        if p.fp:                       # PO2Q_RKF
            ok = p.vr == 1 and C == 64 and not p.nts and p.pd in (2, 3)
            return ("rowsk", 64, p.pd, 0, 0, epi, 0, 0, 1, 0) if ok else None
        if p.pd not in (2, 3) or C not in (32, 64):
            return None
        if C == 64 and p.vr in (1, 2) and not p.nts and (pipe == 1 or (pipe is None and p.vr == 1)):   # PO2Q_RKP
            return ("rowsk", 64, p.pd, int(p.vr == 2), 0, epi, 0, 0, 0, 1)
        if C == 64 and p.vr == 1 and p.nts in (1, 2, 3) and pipe != 0:                                  # PO2Q_RKPN
            return ("rowsk", 64, p.pd, 0, 0, epi, p.nts, 0, 0, 1)
        if p.vr in (1, 2) and not p.nts:                                                                # PO2Q_RK
            return ("rowsk", C, p.pd, int(p.vr == 2), 0, epi, 0, 0, 0, 0)
        if p.vr == 3 and C == 32 and p.pd == 3 and p.nts in (0, 1, 2, 3):                               # PO2Q_RK1 / RKN
            return ("rowsk", 32, 3, 1, 1, epi, p.nts, 0, 0, 0)
        if p.vr == 1 and C == 64 and p.nts in (1, 2, 3):                                                # PO2Q_RKN
            return ("rowsk", 64, p.pd, 0, 0, epi, p.nts, 0, 0, 0)
        return None
    if p.fp:                           # launch_conv_bf16x3_rows: fused staging is for the other three kernels
        return None
    ok = (p.CC, p.NT, p.pd) in ROWS_CFG and p.nts in (0, 1)
    return ("rows", p.CC, p.NT, epi, p.nts, p.pd) if ok else None


def s2ds_pick(shape, mode="po2"):
    """s2ds_plan (po2q_conv_rows2.hip): the candidate po2q_qconv2d_s2ds_f32 runs -- the first stride-2 full-row plan
    with plain stores whose LDS also holds the shortcut's weight, preferring ring depth 4 (C = 16) / 2 (C = 32)."""
    C = shape[1]
    want = 4 if C == 16 else 2
    pick = None
    for i, d in enumerate(plans(shape, mode)):
        p = parse(d)
        if p.kind != "bf16x3_rows" or p.vr != 5 or p.nts != 0 or p.lds + (2 * C // 16) * KIB > LDS_CU:
            continue
        if pick is None or (p.pd == want) > (pick[1].pd == want):
            pick = (i, p)
    return pick


# ---- named geometry conditions: name -> predicate(plan, shape), from the description and the shape alone ----------
def _P(shape):
    return out_size(shape)[0]


def _full(C, nw):
    return lambda p, s: p.vr == 4 and s[1] == C and waves(p, s) == nw


def _k(C, vr):
    return lambda p, s: p.vr == vr and s[1] == C


def _one_segment_of(h):
    return lambda p, s: p.vr in (1, 2, 3) and s[2] == h and p.tilesP == 1 and p.TP == h


CONDS = {
    # conv_rowsf (vr 4)
    "f16_1wave": _full(16, 1), "f16_7waves": _full(16, 7), "f32_1wave": _full(32, 1), "f32_7waves": _full(32, 7),
    "f_W_eq_Wp": lambda p, s: p.vr == 4 and s[3] == p.TQ,
    "f_last_strip_4": lambda p, s: p.vr == 4 and waves(p, s) > 1 and last_strip(p, s) == 4,
    "f_one_segment": lambda p, s: p.vr == 4 and p.tilesP == 1 and p.TP == _P(s),
    "f_last_1row_pd4": lambda p, s: p.vr == 4 and p.pd == 4 and p.tilesP > 1 and last_segment(p, s) == 1,
    "f_last_2rows_pd3": lambda p, s: p.vr == 4 and p.pd == 3 and p.tilesP > 1 and last_segment(p, s) == 2,
    "f_items_not_x8": lambda p, s: p.vr == 4 and items(p, s) > 8 and items(p, s) % 8 != 0,
    "f_items_lt8": lambda p, s: p.vr == 4 and items(p, s) < 8,
    # the residual ring at its largest (C = 32, 7 waves, 4 slots: 157,984 of 163,840 bytes)
    "f_res_ring_max": lambda p, s: p.vr == 4 and rowsf_res_lds(s[1], waves(p, s), p.pd) == rowsf_res_lds(32, 7, 4),
    # conv_rows (vr 0)
    "r16_pd2": lambda p, s: p.vr == 0 and p.CC == 16 and p.pd == 2,
    "r16_pd3": lambda p, s: p.vr == 0 and p.CC == 16 and p.pd == 3,
    "r16_pd6": lambda p, s: p.vr == 0 and p.CC == 16 and p.pd == 6,
    "r32_to_16": lambda p, s: p.vr == 0 and p.CC == 32 and p.NT == 1,
    "r32_to_32": lambda p, s: p.vr == 0 and p.CC == 32 and p.NT == 2,
    "r_items_not_x4": lambda p, s: p.vr == 0 and items(p, s) % 4 != 0,
    "r_ragged_strip": lambda p, s: p.vr == 0 and last_strip(p, s) < p.TQ,
    "r_short_last_segment": lambda p, s: p.vr == 0 and p.tilesP > 1 and last_segment(p, s) < p.TP,
    # conv_rowsk (vr 1 / 2 / 3)
    "k32_vr1": _k(32, 1), "k32_vr2": _k(32, 2), "k32_vr3": _k(32, 3), "k64_vr1": _k(64, 1), "k64_vr2": _k(64, 2),
    "k_pd2": lambda p, s: p.vr in (1, 2, 3) and p.pd == 2,
    "k_pd3": lambda p, s: p.vr in (1, 2, 3) and p.pd == 3,
    "k_nts0": lambda p, s: p.vr in (1, 2, 3) and p.nts == 0, "k_nts1": lambda p, s: p.vr in (1, 2, 3) and p.nts == 1,
    "k_nts2": lambda p, s: p.vr in (1, 2, 3) and p.nts == 2, "k_nts3": lambda p, s: p.vr in (1, 2, 3) and p.nts == 3,
    "k_strips_ragged": lambda p, s: p.vr in (1, 2, 3) and s[3] in (36, 40) and p.tilesQ > 1 and last_strip(p, s) < 32,
    "k_W_le32": lambda p, s: p.vr in (1, 2, 3) and s[3] <= 32 and p.tilesQ == 1,
    "k_H4": _one_segment_of(4), "k_H5": _one_segment_of(5), "k_H6": _one_segment_of(6),
    "k_short_last_segment": lambda p, s: p.vr in (1, 2, 3) and p.tilesP > 1 and last_segment(p, s) < p.TP,
    "k_items_not_x8": lambda p, s: p.vr in (1, 2, 3) and items(p, s) % 8 != 0,
    "k_fp1": lambda p, s: p.vr in (1, 2, 3) and p.fp == 1,
    # conv_rows2 (vr 5)
    "s16_pd2": lambda p, s: p.vr == 5 and s[1] == 16 and p.pd == 2,
    "s16_pd4": lambda p, s: p.vr == 5 and s[1] == 16 and p.pd == 4,
    "s16_nts0": lambda p, s: p.vr == 5 and s[1] == 16 and p.nts == 0,
    "s16_nts1": lambda p, s: p.vr == 5 and s[1] == 16 and p.nts == 1,
    "s16_nd1": lambda p, s: p.vr == 5 and s[1] == 16 and rows2_nd(p, s) == 1,
    "s16_nd2": lambda p, s: p.vr == 5 and s[1] == 16 and rows2_nd(p, s) == 2,
    "s32_nd1": lambda p, s: p.vr == 5 and s[1] == 32 and rows2_nd(p, s) == 1,
    "s32_nd2": lambda p, s: p.vr == 5 and s[1] == 32 and rows2_nd(p, s) == 2,
    "s32_nd3": lambda p, s: p.vr == 5 and s[1] == 32 and rows2_nd(p, s) == 3,
    "s32_nd4": lambda p, s: p.vr == 5 and s[1] == 32 and rows2_nd(p, s) == 4,
    "s_H_odd": lambda p, s: p.vr == 5 and s[2] % 2 == 1, "s_H_even": lambda p, s: p.vr == 5 and s[2] % 2 == 0,
    "s_1wave": lambda p, s: p.vr == 5 and waves(p, s) == 1, "s_7waves": lambda p, s: p.vr == 5 and waves(p, s) == 7,
    "s_one_segment": lambda p, s: p.vr == 5 and p.tilesP == 1,
    "s_short_last_segment": lambda p, s: p.vr == 5 and p.tilesP > 1 and last_segment(p, s) < p.TP,
}
# conditions on how a row is run rather than on its plan: the forms / PIPE settings / flag the row must carry
RUN_CONDS = {
    "k_pipe_unset": lambda r, p: r.shape[1] == 64 and None in r.pipes,
    "k_pipe_0": lambda r, p: r.shape[1] == 64 and 0 in r.pipes,
    "k_pipe_1": lambda r, p: r.shape[1] == 64 and 1 in r.pipes,
    # PO2Q_ROWSK_RES=0 (read once per process: the GPU test runs these rows' residual form in a child process)
    "k_res_switch_off": lambda r, p: r.shape[1] == 64 and r.res_off and res_in_kernel(p, r.shape),
    "s_ds_c16": lambda r, p: r.shape[1] == 16 and "ds" in r.forms and "ds_epi" in r.forms,
    "s_ds_c32": lambda r, p: r.shape[1] == 32 and "ds" in r.forms and "ds_epi" in r.forms,
    "res_in_kernel": lambda r, p: "res" in r.forms and res_in_kernel(p, r.shape),
    "res_by_pass": lambda r, p: "res" in r.forms and not res_in_kernel(p, r.shape),
}
# the guard check (no store outside y) runs on every row that carries one of these
GUARD_CONDS = ("f_last_strip_4", "f_last_1row_pd4", "f_last_2rows_pd3", "f_items_not_x8", "f_items_lt8",
               "r_items_not_x4", "r_ragged_strip", "r_short_last_segment", "k_strips_ragged", "k_short_last_segment",
               "k_items_not_x8", "s_short_last_segment")


# ---- the table -----------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "shape sel forms conds pipes res_off")


def row(shape, sel, forms, conds, pipes=(None,), res_off=False):
    return Row(shape, sel, forms, conds, pipes, res_off)


# (shape, selector, call forms, named conditions[, PO2Q_ROWSK_PIPE settings to run under, PO2Q_ROWSK_RES=0 as well]).
# Every row is the only case of at least one instance or condition (test_every_row_is_needed).  The vr 4 candidates
# crowd conv_rows out of the 40-candidate list wherever they exist, so its C = 16 rows are 228 wide and its
# 32 -> 32 rows 116; conv_rowsk's C = 32 plans survive next to them only where P < 8 leaves one segment height.
ROWS = [
    row((1, 16, 4, 32, 16, 1), dict(vr=4, tile=(4, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_W_eq_Wp', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((1, 16, 4, 196, 16, 1), dict(vr=4, tile=(4, 224), pd=3, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_7waves', 'f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((1, 16, 13, 4, 16, 1), dict(vr=4, tile=(4, 32), pd=4, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_last_1row_pd4', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=0, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=1, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=1, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=2, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=2, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=1, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=1, var=0, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=1, var=1, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=1, var=1, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=3, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=3, var=0, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=3, var=1, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=3, nts=3, var=1, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=0, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=1, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=1, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=2, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=2, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=1, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=1, var=0, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=1, var=1, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=1, var=1, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=3, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=3, var=0, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=3, var=1, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 16, 5, 20, 16, 1), dict(vr=4, tile=(5, 32), pd=4, nts=3, var=1, fp=1), ('plain', 'epi', 'res'), ('f16_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((3, 16, 10, 4, 16, 1), dict(vr=4, tile=(4, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('f16_1wave', 'f_last_2rows_pd3', 'f_items_not_x8', 'res_in_kernel')),
    row((1, 32, 4, 4, 32, 1), dict(vr=4, tile=(4, 16), pd=2, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('f32_1wave', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((1, 32, 4, 100, 32, 1), dict(vr=4, tile=(4, 112), pd=4, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('f32_7waves', 'f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'f_res_ring_max', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=2, nts=0, var=0, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=2, nts=0, var=1, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=2, nts=0, var=1, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=2, nts=2, var=0, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=2, nts=2, var=0, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=2, nts=2, var=1, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=2, nts=2, var=1, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=0, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=1, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=0, var=1, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=2, var=0, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=2, var=0, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=2, var=1, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=3, nts=2, var=1, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=0, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=1, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=4, nts=0, var=1, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=4, nts=2, var=0, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=4, nts=2, var=0, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=4, nts=2, var=1, fp=0), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((2, 32, 5, 20, 32, 1), dict(vr=4, tile=(5, 32), pd=4, nts=2, var=1, fp=1), ('plain', 'epi', 'res'), ('f_last_strip_4', 'f_one_segment', 'f_items_lt8', 'res_in_kernel')),
    row((1, 16, 8, 228, 16, 1), dict(vr=0, tile=(8, 32), pd=2, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('r16_pd2', 'r_ragged_strip', 'res_by_pass')),
    row((1, 16, 8, 228, 16, 1), dict(vr=0, tile=(8, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi'), ('r16_pd3', 'r_ragged_strip')),
    row((1, 16, 8, 228, 16, 1), dict(vr=0, tile=(8, 32), pd=6, nts=0, var=0, fp=0), ('plain', 'epi'), ('r16_pd6', 'r_ragged_strip')),
    row((2, 16, 8, 228, 16, 1), dict(vr=0, tile=(8, 32), pd=2, nts=1, var=0, fp=0), ('plain', 'epi'), ('r16_pd2', 'r_ragged_strip')),
    row((2, 16, 8, 228, 16, 1), dict(vr=0, tile=(8, 32), pd=3, nts=1, var=0, fp=0), ('plain', 'epi'), ('r16_pd3', 'r_ragged_strip')),
    row((2, 16, 8, 228, 16, 1), dict(vr=0, tile=(8, 32), pd=6, nts=1, var=0, fp=0), ('plain', 'epi'), ('r16_pd6', 'r_ragged_strip')),
    row((1, 32, 8, 116, 32, 1), dict(vr=0, tile=(8, 16), pd=2, nts=0, var=0, fp=0), ('plain', 'epi'), ('r32_to_32', 'r_ragged_strip')),
    row((1, 32, 17, 4, 16, 1), dict(vr=0, tile=(9, 16), pd=2, nts=0, var=0, fp=0), ('plain', 'epi'), ('r32_to_16', 'r_items_not_x4', 'r_ragged_strip', 'r_short_last_segment')),
    row((2, 32, 8, 20, 16, 1), dict(vr=0, tile=(8, 16), pd=2, nts=1, var=0, fp=0), ('plain', 'epi'), ('r32_to_16', 'r_ragged_strip')),
    row((2, 32, 8, 116, 32, 1), dict(vr=0, tile=(8, 16), pd=2, nts=1, var=0, fp=0), ('plain', 'epi'), ('r32_to_32', 'r_ragged_strip')),
    row((1, 32, 4, 36, 32, 1), dict(vr=1, tile=(4, 32), pd=2, nts=0, var=0, fp=0), ('plain', 'epi'), ('k32_vr1', 'k_pd2', 'k_nts0', 'k_strips_ragged', 'k_H4', 'k_items_not_x8')),
    row((1, 32, 6, 4, 32, 1), dict(vr=1, tile=(6, 32), pd=2, nts=0, var=0, fp=0), ('plain', 'epi'), ('k32_vr1', 'k_pd2', 'k_nts0', 'k_W_le32', 'k_H6', 'k_items_not_x8')),
    row((2, 32, 5, 20, 32, 1), dict(vr=1, tile=(5, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi'), ('k32_vr1', 'k_pd3', 'k_nts0', 'k_W_le32', 'k_H5', 'k_items_not_x8')),
    row((1, 64, 4, 4, 64, 1), dict(vr=1, tile=(4, 32), pd=2, nts=0, var=0, fp=1), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd2', 'k_nts0', 'k_W_le32', 'k_H4', 'k_items_not_x8', 'k_fp1', 'k_pipe_unset', 'res_in_kernel')),
    row((1, 64, 7, 4, 64, 1), dict(vr=1, tile=(4, 32), pd=2, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd2', 'k_nts0', 'k_W_le32', 'k_short_last_segment', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=2, nts=1, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd2', 'k_nts1', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=2, nts=2, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd2', 'k_nts2', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=2, nts=3, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd2', 'k_nts3', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd3', 'k_nts0', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=3, nts=0, var=0, fp=1), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd3', 'k_nts0', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_fp1', 'k_pipe_unset', 'res_in_kernel')),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=3, nts=1, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd3', 'k_nts1', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=3, nts=2, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd3', 'k_nts2', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((2, 64, 5, 20, 64, 1), dict(vr=1, tile=(5, 32), pd=3, nts=3, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr1', 'k_pd3', 'k_nts3', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_0', 'res_in_kernel'), pipes=(None, 0)),
    row((1, 32, 4, 4, 32, 1), dict(vr=2, tile=(4, 32), pd=2, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('k32_vr2', 'k_pd2', 'k_nts0', 'k_W_le32', 'k_H4', 'k_items_not_x8', 'res_by_pass')),
    row((2, 32, 5, 20, 32, 1), dict(vr=2, tile=(5, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi'), ('k32_vr2', 'k_pd3', 'k_nts0', 'k_W_le32', 'k_H5', 'k_items_not_x8')),
    row((1, 64, 4, 4, 64, 1), dict(vr=2, tile=(4, 32), pd=2, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr2', 'k_pd2', 'k_nts0', 'k_W_le32', 'k_H4', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_1', 'k_res_switch_off', 'res_in_kernel'), pipes=(None, 1), res_off=True),
    row((2, 64, 5, 20, 64, 1), dict(vr=2, tile=(5, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('k64_vr2', 'k_pd3', 'k_nts0', 'k_W_le32', 'k_H5', 'k_items_not_x8', 'k_pipe_unset', 'k_pipe_1', 'res_in_kernel'), pipes=(None, 1)),
    row((1, 32, 4, 4, 32, 1), dict(vr=3, tile=(4, 32), pd=3, nts=0, var=0, fp=0), ('plain', 'epi', 'res'), ('k32_vr3', 'k_pd3', 'k_nts0', 'k_W_le32', 'k_H4', 'k_items_not_x8', 'res_in_kernel')),
    row((1, 32, 4, 4, 32, 1), dict(vr=3, tile=(4, 32), pd=3, nts=1, var=0, fp=0), ('plain', 'epi', 'res'), ('k32_vr3', 'k_pd3', 'k_nts1', 'k_W_le32', 'k_H4', 'k_items_not_x8', 'res_in_kernel')),
    row((1, 32, 4, 4, 32, 1), dict(vr=3, tile=(4, 32), pd=3, nts=2, var=0, fp=0), ('plain', 'epi', 'res'), ('k32_vr3', 'k_pd3', 'k_nts2', 'k_W_le32', 'k_H4', 'k_items_not_x8', 'res_in_kernel')),
    row((1, 32, 4, 4, 32, 1), dict(vr=3, tile=(4, 32), pd=3, nts=3, var=0, fp=0), ('plain', 'epi', 'res'), ('k32_vr3', 'k_pd3', 'k_nts3', 'k_W_le32', 'k_H4', 'k_items_not_x8', 'res_in_kernel')),
    row((1, 16, 4, 8, 32, 2), dict(vr=5, tile=(2, 16), pd=2, nts=1, var=0, fp=1), ('plain', 'epi'), ('s16_pd2', 's16_nts1', 's16_nd1', 's_H_even', 's_1wave', 's_one_segment')),
    row((1, 16, 4, 8, 32, 2), dict(vr=5, tile=(2, 16), pd=4, nts=0, var=0, fp=1), ('plain', 'epi', 'ds', 'ds_epi'), ('s16_pd4', 's16_nts0', 's16_nd1', 's_H_even', 's_1wave', 's_one_segment', 's_ds_c16')),
    row((1, 16, 4, 8, 32, 2), dict(vr=5, tile=(2, 16), pd=4, nts=1, var=0, fp=1), ('plain', 'epi'), ('s16_pd4', 's16_nts1', 's16_nd1', 's_H_even', 's_1wave', 's_one_segment')),
    row((1, 16, 4, 200, 32, 2), dict(vr=5, tile=(2, 112), pd=2, nts=0, var=0, fp=1), ('plain', 'epi'), ('s16_pd2', 's16_nts0', 's16_nd2', 's_H_even', 's_7waves', 's_one_segment')),
    row((1, 16, 17, 8, 32, 2), dict(vr=5, tile=(5, 16), pd=2, nts=0, var=0, fp=1), ('plain', 'epi'), ('s16_pd2', 's16_nts0', 's16_nd1', 's_H_odd', 's_1wave', 's_short_last_segment')),
    row((2, 16, 5, 24, 32, 2), dict(vr=5, tile=(3, 16), pd=2, nts=1, var=0, fp=1), ('plain', 'epi'), ('s16_pd2', 's16_nts1', 's16_nd2', 's_H_odd', 's_1wave', 's_one_segment')),
    row((2, 16, 5, 24, 32, 2), dict(vr=5, tile=(3, 16), pd=4, nts=0, var=0, fp=1), ('plain', 'epi', 'ds', 'ds_epi'), ('s16_pd4', 's16_nts0', 's16_nd2', 's_H_odd', 's_1wave', 's_one_segment', 's_ds_c16')),
    row((2, 16, 5, 24, 32, 2), dict(vr=5, tile=(3, 16), pd=4, nts=1, var=0, fp=1), ('plain', 'epi'), ('s16_pd4', 's16_nts1', 's16_nd2', 's_H_odd', 's_1wave', 's_one_segment')),
    row((1, 32, 4, 8, 64, 2), dict(vr=5, tile=(2, 16), pd=2, nts=0, var=0, fp=1), ('plain', 'epi', 'ds', 'ds_epi'), ('s32_nd1', 's_H_even', 's_1wave', 's_one_segment', 's_ds_c32')),
    row((1, 32, 4, 16, 64, 2), dict(vr=5, tile=(2, 16), pd=2, nts=0, var=0, fp=1), ('plain', 'epi', 'ds', 'ds_epi'), ('s32_nd2', 's_H_even', 's_1wave', 's_one_segment', 's_ds_c32')),
    row((2, 32, 5, 24, 64, 2), dict(vr=5, tile=(3, 16), pd=2, nts=0, var=0, fp=1), ('plain', 'epi', 'ds', 'ds_epi'), ('s32_nd3', 's_H_odd', 's_1wave', 's_one_segment', 's_ds_c32')),
    row((2, 32, 5, 32, 64, 2), dict(vr=5, tile=(3, 16), pd=2, nts=0, var=0, fp=1), ('plain', 'epi', 'ds', 'ds_epi'), ('s32_nd4', 's_H_odd', 's_1wave', 's_one_segment', 's_ds_c32')),
]

# shapes too short for a row kernel (its planner starts at 4 rows per segment, conv_rows' at 8): (shape, the plan
# vr values that must be absent).  The GPU test runs their default plan, whichever kernel that is.
FALLBACK_SHAPES = [
    ((2, 16, 3, 36, 16, 1), (4, 0)),      # P < 4: no full-row plan (and none of conv_rows)
    ((2, 32, 3, 36, 32, 1), (4, 1, 2, 3, 0)),
    ((2, 32, 7, 36, 16, 1), (0,)),        # 32 -> 16, P < 8: conv_rows is the only row kernel of the pair, and refuses
    ((2, 16, 7, 228, 16, 1), (0, 4)),     # P < 8 on a row too wide for the full-row kernel
]


def row_id(r):
    s = r.sel
    return "%s-vr%d-%dx%d-pd%d-nts%d-var%d-fp%d" % ("x".join(map(str, r.shape)), s["vr"], s["tile"][0], s["tile"][1],
                                                    s["pd"], s["nts"], s["var"], s["fp"])


def matches(p, sel):
    return p.kind == "bf16x3_rows" and all(
        ((p.TP, p.TQ) if k == "tile" else (p.tilesP, p.tilesQ) if k == "tiles" else getattr(p, k)) == v
        for k, v in sel.items())


def find_plan(r, mode="po2", sel=None):
    """(candidate index, Plan) of the row's plan among _lib.plans of its shape, or None."""
    for i, d in enumerate(plans(r.shape, mode)):
        if "kind=bf16x3_rows" in d and matches(parse(d), sel or r.sel):
            return i, parse(d)
    return None


def row_keys(r, p):
    """(form, PIPE setting) -> instance key, for everything the GPU test runs of row r."""
    return {(f, pipe): dispatch(p, r.shape, f, pipe)
            for f in r.forms for pipe in (r.pipes if f in ("plain", "epi") else (None,))}


def siblings(r):
    """Selectors of the plans that must give bit for bit the row's output: nts = 0 (cache policy only) and fp = 0
    (the same weight, packed by another kernel)."""
    out = []
    if r.sel["nts"]:
        out.append(dict(r.sel, nts=0))
    if r.sel["fp"] and r.sel["vr"] != 5:     # conv_rows2 has no pre-packed form
        out.append(dict(r.sel, fp=0))
    return out
