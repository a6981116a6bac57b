"""CPU: the case tables of tests/_tile_cases.py reach every instance of the general-geometry fp32-forward kernels
that the planners can produce, every row's forced tile is the plan that runs, and the named geometry conditions
are met -- all from the planner's own descriptions (host only).  tests/test_gpu_tile_paths.py runs the rows.

The reachable instance sets are written out here as rules restating the planners' caps (x3_candidates,
x3p_candidates, plan_fallback); they are not obtained from the planner.  What the launch dispatch could
instantiate beyond them is listed with the cap that forbids it, and a knob sweep checks it is really refused."""
import itertools
import json
import os

import pytest

from po2_quantization_amd import _lib
from tests import _tile_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))
kThreads, kXI, kWI = 256, 3, 5            # po2q_conv_x3.hip
kPMaxNI, kPMaxNW, kPXS = 8, 8, 3          # po2q_conv_x3p.hip


def cdiv(a, b):
    return -(-a // b)


# ---- conv_bf16x3<CC, NT, NJ, KS, MC, PD> -------------------------------------------------------------------------
def x3_launchable():
    """What launch_conv_bf16x3 can instantiate: NJ = 7 only with NT = 1 (launch_x3_nj) and PD = 1 (launch_x3),
    KS = 5 only with CC = 16 (launch_x3_ks)."""
    out = set()
    for cc, nt, nj, ks, mc, pd in itertools.product((16, 32), (1, 2, 4), (1, 2, 4, 7), (1, 5, 0), (0, 1), (1, 2)):
        if (nj == 7 and (nt != 1 or pd != 1)) or (ks == 5 and cc != 16):
            continue
        out.add((cc, nt, nj, ks, mc, pd))
    return out


def x3_refusal(key):
    """The x3_candidates condition that keeps the planner from ever producing `key`, or None.  A tile of 64 * NJ
    output pixels has at least as many halo pixels (HH >= TP, WW >= TQ), each staged as CC / 8 channel octets."""
    cc, nt, nj, ks, mc, pd = key
    if cc == 32 and ks != 1:
        return "CC = 32 only for taps == 1 (with C > 16), where ksteps = cdiv(taps * 4, 4) = 1"
    if 64 * nj * (cc // 8) > kXI * kThreads:
        return "HH * WW * (CC / 8) = %d+ staged items > kXI * kThreads = %d" % (64 * nj * (cc // 8), kXI * kThreads)
    # everything else is reachable: NT from K (1 / 2 / 4 survive ksteps * NT <= 20 for ksteps <= 5 / 10 / 20),
    # KS from the tap count (1: 1 or 2 taps; 5: 9 or 10; 0: the rest up to 40), MC from C > CC or K > 16 * NT
    # (CC = 16 with one tap has C <= 16, so there MC needs K > 64, NT = 4 -- or two taps), PD free for NJ <= 4
    return None


# ---- conv_x3p<waves, NT, NJ, vr, KS, MC, OV> -----------------------------------------------------------------------
def dma_launchable():
    """What launch_conv_bf16x3_dma can instantiate: vr in {1, 2, 4, 8} <= waves with NT = 1 and KS = 0
    (launch_p_w), else KS in {5, 0} (launch_p_k); MC and OV either way (launch_p)."""
    out = set()
    for wv, nj, mc, ov in itertools.product((4, 8), (1, 2, 4), (0, 1), (0, 1)):
        for vr in (1, 2, 4, 8):
            if vr <= wv:
                out.add((wv, 1, nj, vr, 0, mc, ov))
        for nt, ks in itertools.product((1, 2, 4), (5, 0)):
            out.add((wv, nt, nj, 0, ks, mc, ov))
    return out


def dma_refusal(key):
    """The x3p_candidates caps that forbid `key` for every geometry, or None when some geometry passes them all.
    The smallest footprint of an instance is stride 1, dilation 1, a window that starts 16-byte aligned (d0 = 0)
    and one resident weight chunk; the kernel is 3x3 for vr > 0, any 9- or 10-tap shape for KS = 5 and 1x1 for
    KS = 0 (a larger stride, dilation, d0 or chunk count only adds halo, DMA chunks or LDS).  MC = 1 needs several
    chunks or k-blocks, which costs a streamed instance nothing (its ring slots do not grow with them)."""
    wv, nt, nj, vr, ks, mc, ov = key
    px = 16 * wv * nj
    if vr:
        kernels, tiles = [(3, 3)], [(nj * (wv // vr), 16 * vr)]
    else:
        kernels = [(3, 3), (1, 9), (9, 1), (2, 5), (5, 2), (1, 10), (10, 1)] if ks == 5 else [(1, 1)]
        tiles = [(px // tq, tq) for tq in range(4, px + 1, 4) if px % tq == 0]
    caps = set()
    for R, S in kernels:
        steps = 15 if vr else cdiv(R * S * 2, 4)
        if steps * nt * 64 > kPMaxNW * 4 * 64:
            caps.add("NT halved: ksteps * NT * 64 > kPMaxNW * 256")
            continue
        for tp, tq in tiles:
            HH, WW = tp + R - 1, tq + S - 1
            nck = cdiv(WW, 4)
            ni = cdiv(16 * HH * nck, 64 * wv)
            if ni > kPMaxNI:
                caps.add("x DMA instructions per wave: ni > kPMaxNI")
                continue
            if cdiv(HH * WW * 2, 64 * wv) > kPXS:
                caps.add("split items per thread > kPXS")
                continue
            plane, raw, wfr = HH * WW * 32 + 32, ni * wv * 1024, steps * nt * 64
            nw = cdiv(wfr, 64 * wv)
            if mc and nw > kPMaxNW:
                caps.add("weight DMA instructions per wave: nw > kPMaxNW")
                continue
            w_slot = nw * wv * 1024 if mc else wfr * 16
            lds = (6 if ov else 3) * plane + (3 if ov else 2) * raw + (3 if mc else 1) * w_slot + 4096 + 256
            if lds > 160 * 1024:
                caps.add("LDS > 160 KiB")
                continue
            return None
    return "; ".join(sorted(caps))


MFMA_EVERY = set(itertools.product((1, 2, 4), (1, 2, 4)))  # launch_conv: MI from Kg, NJ from P * Q, independent


def _found(rows):
    out = []
    for row in rows:
        f = T.find_plan(row)
        assert f is not None, ("the planner ignored the forced tile, or the candidate list no longer holds this "
                               "instance: %s %s" % (T.row_kind(row), T.row_id(row)), row[2])
        out.append((row, f[1]))
    return out


@pytest.fixture(scope="module")
def tile_plans():
    return _found(T.X3_ROWS + T.X3_EDGES + T.DMA_ROWS + T.DMA_EDGES)


@pytest.mark.parametrize("kind,launchable,refusal,rows", [
    ("bf16x3", x3_launchable, x3_refusal, T.X3_ROWS + T.X3_EDGES),
    ("bf16x3_dma", dma_launchable, dma_refusal, T.DMA_ROWS + T.DMA_EDGES),
])
def test_rows_reach_exactly_the_reachable_instances(kind, launchable, refusal, rows):
    every = launchable()
    unreachable = {k: refusal(k) for k in every if refusal(k)}
    expected = every - set(unreachable)
    reached = {tuple(row[2]) for row in rows}
    for row in rows:  # the forced tile is the plan that runs, with the row's instance key, in both modes
        for mode in ("po2", "po2+"):
            assert T.find_plan(row, mode) is not None, (kind, T.row_id(row), row[2], mode)
    print("%s: %d instances reached, %d the dispatch can launch, %d unreachable" %
          (kind, len(reached), len(every), len(unreachable)))
    for k in sorted(unreachable):
        print("  unreachable %s: %s" % (k, unreachable[k]))
    missing = sorted(expected - reached)
    assert not missing, "no %s row reaches the instances %s" % (kind, missing)
    assert reached == expected, "%s rows outside the reachable set: %s" % (kind, sorted(reached - expected))


PROBE_KERNELS = [(1, 1), (1, 2), (2, 2), (3, 3), (2, 5), (5, 5)]


def _probe_keys(kind, envs):
    """Instance keys of `kind` over a sweep of shapes under each forced-tile environment."""
    seen = set()
    for (R, S), C, K, W, pad in itertools.product(PROBE_KERNELS, (8, 24, 40), (16, 40), (20, 68, 132), (0, 1)):
        if pad and R * S == 1:
            continue
        shape = (2, C, 40, W, K, R, S, 1, 1, pad * (R // 2), pad * (S // 2), 1, 1)
        for env in envs:
            for d in T.plans(shape, env):
                p = T.parse(d)
                if p.kind == kind:
                    seen.add(T.instance_key(p))
    return seen


def test_unreachable_x3_instances_are_refused():
    """Forcing every 256- and 448-pixel tile never yields NJ = 7, nor NJ = 4 or a general tap count with CC = 32:
    the planner drops the override (an invalid forced tile is ignored) and plans another instance."""
    envs = [{"PO2Q_X3_TILE": "%d,%d,%d" % (nj, 64 * nj // tq, tq)} for nj in (4, 7) for tq in (4, 8, 16, 32, 64)
            if (64 * nj) % tq == 0]
    seen = _probe_keys("bf16x3", envs + [{}])
    bad = sorted(k for k in seen if x3_refusal(k))
    assert not bad, bad
    assert seen <= x3_launchable()
    assert any(k[0] == 32 for k in seen) and any(k[2] == 4 for k in seen)  # the sweep does reach their neighbours


def test_unreachable_dma_instances_are_refused():
    unreachable = sorted(k for k in dma_launchable() if dma_refusal(k))
    envs = []
    for wv, nt, nj, vr, ks, mc, ov in unreachable:
        px = 16 * wv * nj
        tiles = [(nj * (wv // vr), 16 * vr)] if vr else [(px // tq, tq) for tq in (4, 8, 16, 32, 64) if px % tq == 0]
        for tp, tq in tiles:
            env = {"PO2Q_X3P_WAVES": str(wv), "PO2Q_X3P_TILE": "%d,%d,%d,%d" % (nj, tp, tq, vr)}
            if env not in envs:
                envs.append(env)
    seen = _probe_keys("bf16x3_dma", envs)
    bad = sorted(k for k in seen if dma_refusal(k))
    assert not bad, bad
    assert seen <= dma_launchable()
    assert seen, "the sweep planned no DMA candidate at all"


def test_tap_cap_of_the_tile_kernels():
    """40 taps (20 k-steps) is the most either tile kernel runs; 42 taps fall back to the fp32 MFMA kernel."""
    for rows, kind in ((T.X3_ROWS, "bf16x3"), (T.DMA_ROWS, "bf16x3_dma")):
        most = max(r[0][5] * r[0][6] for r in rows)
        assert most == T.MOST_TAPS, (kind, most)
    assert kWI * kThreads // 64 == cdiv(T.MOST_TAPS * 2, 4)
    for mode in ("po2", "po2+"):
        ds = T.plans(T.FIRST_FALLBACK_TAPS, mode=mode)
        assert [T.parse(d).kind for d in ds] == ["mfma_f32"], ds


# ---- named conditions: name -> (predicate of (shape, Plan), kinds that must meet it) ---------------------------------
BOTH = ("bf16x3", "bf16x3_dma")


def _pq(s):
    return T.out_size(s)


def _vec(s, p):
    return _pq(s)[1] % 4 == 0 and p.TQ % 4 == 0


CONDITIONS = {
    "vec = 0 (scalar epilogue stores)": (lambda s, p: not _vec(s, p), BOTH),
    "vec = 1 (float4 epilogue stores)": (_vec, BOTH),
    "remap = 0 (blocks % 8 != 0)": (lambda s, p: p.blocks % 8 != 0, BOTH),
    "remap = 1 (blocks % 8 == 0)": (lambda s, p: p.blocks % 8 == 0, BOTH),
    "K % 16 != 0": (lambda s, p: s[4] % 16 != 0, BOTH),
    "K % (16 NT) != 0 with kblocks > 1": (lambda s, p: s[4] % (16 * p.NT) != 0 and p.kblocks > 1, BOTH),
    "C < 8": (lambda s, p: s[1] < 8, BOTH),
    "C % 8 != 0": (lambda s, p: s[1] % 8 != 0, BOTH),
    "C % 16 != 0 with chunks > 1": (lambda s, p: s[1] % 16 != 0 and p.chunks > 1, BOTH),
    "CC = 32 with a ragged second chunk": (lambda s, p: p.CC == 32 and p.chunks > 1 and s[1] % 32 != 0, ("bf16x3",)),
    "chunks * kblocks >= 4 with streamed weights (the ring wraps in one tile)":
        (lambda s, p: p.wstream == 1 and p.chunks * p.kblocks >= 4, BOTH),
    "ragged last tile in P": (lambda s, p: p.tilesP > 1 and _pq(s)[0] % p.TP != 0, BOTH),
    "ragged last tile in Q": (lambda s, p: p.tilesQ > 1 and _pq(s)[1] % p.TQ != 0, BOTH),
    "one tile larger than the image": (lambda s, p: p.tilesP * p.tilesQ == 1 and p.TP * p.TQ > _pq(s)[0] * _pq(s)[1],
                                       BOTH),
    "sh != sw": (lambda s, p: s[7] != s[8], BOTH),
    "dh != dw": (lambda s, p: s[11] != s[12], BOTH),
    "ph != pw": (lambda s, p: s[9] != s[10], BOTH),
    "pad 0 with R > 1 and S > 1": (lambda s, p: s[9] == 0 and s[10] == 0 and s[5] > 1 and s[6] > 1, BOTH),
    "ph > (R - 1) dh: output rows of padding only": (lambda s, p: s[5] > 1 and s[9] > (s[5] - 1) * s[11], BOTH),
    "pw > (S - 1) dw: output columns of padding only": (lambda s, p: s[6] > 1 and s[10] > (s[6] - 1) * s[12], BOTH),
    "1x3": (lambda s, p: (s[5], s[6]) == (1, 3), BOTH),
    "3x1": (lambda s, p: (s[5], s[6]) == (3, 1), BOTH),
    "R != S beyond 1x3 / 3x1": (lambda s, p: s[5] != s[6] and s[5] * s[6] > 3, BOTH),
    "2x2 (even tap count, no padded k-slot)": (lambda s, p: (s[5], s[6]) == (2, 2), BOTH),
    "4x4": (lambda s, p: (s[5], s[6]) == (4, 4), BOTH),
    "6x6": (lambda s, p: (s[5], s[6]) == (6, 6), BOTH),
    "an odd tap count above 1 (a padded k-slot)": (lambda s, p: s[5] * s[6] > 1 and (s[5] * s[6]) % 2 == 1, BOTH),
    "%d taps, the cap" % T.MOST_TAPS: (lambda s, p: s[5] * s[6] == T.MOST_TAPS, BOTH),
}
for _d0 in range(4):  # w0 - (16-byte aligned window start), floats: x3p_candidates' d0 = (4 - pw % 4) % 4
    CONDITIONS["DMA window alignment d0 = %d" % _d0] = (lambda s, p, d=_d0: (4 - s[10] % 4) % 4 == d, ("bf16x3_dma",))


def test_rows_meet_every_named_condition(tile_plans):
    unmet = []
    for name, (cond, kinds) in CONDITIONS.items():
        for kind in kinds:
            hits = [T.row_id(r) for r, p in tile_plans if T.row_kind(r) == kind and cond(r[0], p)]
            print("%s [%s]: %d rows, e.g. %s" % (name, kind, len(hits), hits[:2]))
            if not hits:
                unmet.append((name, kind))
    assert not unmet, "no row meets: %s" % unmet
    assert all(r[0][0] > 1 for r, _ in tile_plans), "every row runs a batch (N > 1)"


def test_described_plans_match_their_shapes(tile_plans):
    """What the describe line says of each row follows from the shape: chunk, k-block and k-step counts."""
    for row, p in tile_plans:
        s = row[0]
        assert p.chunks == cdiv(s[1], p.CC) and p.kblocks == cdiv(s[4], 16 * p.NT), (row, p)
        assert p.tilesP == cdiv(_pq(s)[0], p.TP) and p.tilesQ == cdiv(_pq(s)[1], p.TQ), (row, p)
        assert p.blocks == s[0] * p.kblocks * p.tilesP * p.tilesQ, (row, p)
        if not p.vr:
            assert p.ksteps == cdiv(s[5] * s[6] * (p.CC // 8), 4), (row, p)


# ---- the other rows the GPU tests run -------------------------------------------------------------------------------
def test_special_rows_are_the_plans_that_run():
    for row in T.MULTI_ITEM_ROWS + T.NEIGHBOUR_TILE_ROWS + T.ALIGNED_ROWS:
        assert T.find_plan(row) is not None, row
    for kind in BOTH:
        mi = [r for r in T.MULTI_ITEM_ROWS if T.row_kind(r) == kind]
        general = [r for r in mi if r[0][5:7] == (5, 5)]
        strided = [r for r in mi if r[0][5:9] == (3, 3, 2, 1)]
        ks = 3 if kind == "bf16x3" else 4
        mcf = 4 if kind == "bf16x3" else 5
        for rows, want in ((general, 0), (strided, 5)):
            assert {r[2][ks] for r in rows} == {want}, (kind, rows)
            assert {r[2][mcf] for r in rows} == {0, 1}, (kind, rows)
            if kind == "bf16x3_dma":
                assert {(r[2][5], r[2][6]) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}, rows
    for row in T.ALIGNED_ROWS:
        assert _vec(row[0], T.find_plan(row)[1]), row
    assert {T.row_kind(r) for r in T.ALIGNED_ROWS} == set(BOTH)
    for row in T.NEIGHBOUR_TILE_ROWS:
        s = row[0]
        assert s[0] == 1 and s[1] < 16 and s[1] % 8 != 0 and s[9] > 0 and s[10] > 0, row
    for rows in (T.FUSED_TILE_ROWS, [(r[0],) for r in T.FUSED_MFMA_ROWS], [(s,) for s in T.FUSED_DEPTHWISE_ROWS]):
        pq = {(_pq(r[0])[0] * _pq(r[0])[1]) % 4 == 0 for r in rows}
        assert pq == {False, True}, rows  # epilogue_kernel_scalar and the float4 epilogue kernel
    assert {T.row_kind(r) for r in T.FUSED_TILE_ROWS} == set(BOTH)
    assert {T.row_kind(r) for r in T.WINDOW_ROWS} == set(BOTH)
    for row in T.WINDOW_ROWS + T.NONFINITE_TILE_ROWS:
        assert row[2][3 if T.row_kind(row) == "bf16x3" else 4] == 0, row  # the runtime tap table
        for bits, fsr in ((1, 1), (2, 1), (7, 1), (4, 2)):
            assert T.find_plan(row, "po2", bits, fsr) is not None, (row, bits, fsr)
    # bits = 8: the window's bottom 2^-127 is no normal bf16, both planners refuse and the fp32 MFMA kernel runs
    for row in T.WINDOW_ROWS:
        ds = T.plans(row[0], bits=8)
        assert [T.parse(d).kind for d in ds] == ["mfma_f32"], ds
        with pytest.raises(_lib.Po2qError, match="bf16x3"):
            T.plans(row[0], bits=8, precision="bf16x3")


def test_mfma_rows_reach_every_instance_and_condition():
    plans = []
    for shape, prec, key in T.MFMA_ROWS + [T.NEIGHBOUR_MFMA]:
        for mode in ("po2", "po2+"):
            p = T.parse(T.describe(shape, mode=mode, precision=prec))
            assert p.kind == "mfma_f32" and T.instance_key(p) == key, (shape, prec, p)
        plans.append((shape, p))
    reached = {T.instance_key(p) for _, p in plans}
    print("mfma_f32: %d instances reached, %d the dispatch can launch, 0 unreachable" % (len(reached), len(MFMA_EVERY)))
    assert reached == MFMA_EVERY, sorted(MFMA_EVERY - reached)
    conds = {
        "nchunks > 1": lambda s, p: p.chunks > 1,
        "Cg % 4 != 0": lambda s, p: (s[1] // s[13]) % 4 != 0,
        "Kg % 16 != 0": lambda s, p: (s[4] // s[13]) % 16 != 0,
        "groups = 2": lambda s, p: s[13] == 2,
        "groups = 4": lambda s, p: s[13] == 4,
        "stride 2 (plane stride padded to an odd bank offset)": lambda s, p: s[8] == 2,
        "7x7": lambda s, p: (s[5], s[6]) == (7, 7),
        "9x9 (above 64 taps)": lambda s, p: (s[5], s[6]) == (9, 9),
        "ragged last tile": lambda s, p: _pq(s)[0] % p.TP != 0 or _pq(s)[1] % p.TQ != 0,
        "sh != sw and ph != pw": lambda s, p: s[7] != s[8] and s[9] != s[10],
    }
    unmet = [n for n, c in conds.items() if not any(c(s, p) for s, p in plans)]
    assert not unmet, unmet
    # above the tile kernels' tap cap (and for grouped convs) the fp32 MFMA kernel is the only candidate
    for shape, prec, _ in T.MFMA_ROWS:
        if prec == "auto":
            assert len(T.plans(shape)) == 1, shape


def test_depthwise_rows_run_the_legacy_kernel():
    for shape in T.DEPTHWISE_ROWS + [T.NEIGHBOUR_DEPTHWISE]:
        for mode in ("po2", "po2+"):
            assert T.describe(shape, mode=mode).startswith("kind=depthwise CC=1 NT=0 MI=1 NJ=1 vr=0 "), shape
    s = T.DEPTHWISE_ROWS
    assert s[0][4] == 2 * s[0][1] and s[1][5:7] == (5, 5) and s[2][5:7] == (3, 5) and s[3][11:13] == (2, 2)
    assert s[4][9:11] == (0, 0) and s[5][7:9] == (2, 1)


# ---- the LDS-fit boundary of the fp32 MFMA kernel ------------------------------------------------------------------
def test_stem_plans_with_a_halved_pixel_tile():
    """7x7 / stride 2 / C = 3 -> K = 64 (the ImageNet stem): 256 output pixels give NJ = 4, whose 37x37 halo plus
    49 KiB of weights exceed 64 KiB at the smallest channel chunk; plan_fallback retries with NJ = 2 (an 8x16 tile,
    halo 21x37), which fits.  The same layer at full size plans the same tile."""
    for shape in (T.STEM, (256, 3, 224, 224, 64, 7, 7, 2, 2, 3, 3, 1, 1, 1)):
        for mode in ("po2", "po2+", "none"):
            p = T.parse(T.describe(shape, mode=mode))
            assert (p.kind, p.MI, p.NJ, p.TP, p.TQ, p.HH, p.WW, p.CC) == ("mfma_f32", 4, 2, 8, 16, 21, 37, 4), p
            assert p.lds <= 64 * 1024
    # neighbours that planned before keep NJ = 4
    assert T.parse(T.describe((2, 3, 32, 32, 16, 7, 7, 2, 2, 3, 3, 1, 1, 1))).NJ == 4
    assert T.parse(T.describe((2, 8, 32, 32, 64, 7, 7, 1, 1, 3, 3, 1, 1, 1))).NJ == 4


def test_largest_kernel_of_the_fp32_mfma_kernel():
    """With MI = 4 a chunk's weights are taps KiB: 8x8 cannot fit beside any halo and is refused on the host, by
    the describe and the workspace query alike; 7x7 is the largest square kernel that plans."""
    with pytest.raises(_lib.Po2qError, match=r"conv tile does not fit in LDS \(kernel too large\)"):
        T.describe(T.MFMA_TOO_LARGE)
    g13, groups = T.geom(T.MFMA_TOO_LARGE)
    assert _lib.load().po2q_qconv2d_workspace_bytes(*g13, groups, 4, 1, 1, 0) == 0
    p = T.parse(T.describe(T.MFMA_LARGEST))
    assert p.kind == "mfma_f32" and p.MI == 4


def test_retry_changes_no_plan_that_fitted_before():
    """The describe lines of tests/test_gpu_conv.py's SHAPES in every mode and precision, recorded before
    plan_fallback learned to shrink its pixel tile (tests/golden/conv_shapes_describe.json), byte for byte."""
    import ast
    import re

    with open(os.path.join(HERE, "test_gpu_conv.py")) as f:
        m = re.search(r"^SHAPES = \[(.*?)^\]", f.read(), re.S | re.M)
    shapes = ast.literal_eval("[" + m.group(1) + "]")
    with open(os.path.join(HERE, "golden", "conv_shapes_describe.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 9 * len(shapes)
    for s in shapes:
        N, C, H, W, K, R, S, st, pad, dil, g = s
        for mode in ("po2", "po2+", "none"):
            for prec in ("auto", "fp32", "bf16x3"):
                try:
                    with T.knobs({}):
                        d = _lib.describe(N, C, H, W, K, R, S, st, pad, dil, g, 4, mode, 1, prec)
                except _lib.Po2qError as e:
                    d = "error: " + str(e)
                assert d == recorded["%s|%s|%s" % (str(s), mode, prec)], (s, mode, prec)
