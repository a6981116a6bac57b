"""GPU: every producible instance of the four row-streaming kernels behind kind bf16x3_rows -- conv_rows, conv_rowsf,
conv_rowsk, conv_rows2 -- through the rows of tests/_rows_cases.py, against the oracle (fp64 direct conv of the
bit-exact Q(w)) at the project's parity bar CONV_TOL (normwise: max |diff| / max |ref| over the whole output).
tests/test_rows_cases_cpu.py proves on the host that the rows reach every instance and geometry condition; here
each row's plan is looked up the same way and run by its candidate index through the C ABI, which plans on every
call (po2q_qconv2d_f32_plan; po2q_qconv2d_fused_f32 under PO2Q_PLAN for the epilogue and residual forms)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from po2_quantization_amd import _lib
from tests import _rows_cases as R
from tests import _tile_cases as T
from tests._util import CONV_TOL, normwise_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("po2", "po2+")
ACTS = ("relu", "none", "silu", "relu6")
CHUNK = 6
GUARD = 1024      # floats (4 KiB) of sentinel on either side of y
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and both modes' oracle outputs of a shape, computed once and shared by all its rows (read-only)."""
    N, C, H, W, K, st = shape
    P, Q = R.out_size(shape)
    g = torch.Generator().manual_seed(sum(shape) * 7 + W)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * 0.1
    b = torch.randn(K, generator=g) * 0.1
    ps, pb = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    res = torch.randn(N, K, P, Q, generator=g)
    ref = {m: T.reference(x, w, R.shape13(shape), m) for m in MODES}
    host = dict(x=x, w=w, b=b, ps=ps, pb=pb, res=res)
    return host, {k: v.to(DEV) for k, v in host.items()}, ref


@functools.lru_cache(maxsize=None)
def _case_ds(shape, mode):
    """The shortcut's 1x1 stride-2 weight and oracle output."""
    N, C, H, W, K, st = shape
    g = torch.Generator().manual_seed(sum(shape))
    wds = torch.randn(K, C, 1, 1, generator=g) * 0.2
    x = _case(shape)[0]["x"]
    ref = T.reference(x, wds, (N, C, H, W, K, 1, 1, 2, 2, 0, 0, 1, 1), mode)
    return wds, ref


class _env:
    """PO2Q_ROWSK_PIPE for the duration of a launch (read at every launch_conv_rowsk call)."""

    def __init__(self, pipe):
        self.pipe = pipe

    def __enter__(self):
        self.saved = os.environ.pop("PO2Q_ROWSK_PIPE", None)
        if self.pipe is not None:
            os.environ["PO2Q_ROWSK_PIPE"] = str(self.pipe)

    def __exit__(self, *a):
        os.environ.pop("PO2Q_ROWSK_PIPE", None)
        if self.saved is not None:
            os.environ["PO2Q_ROWSK_PIPE"] = self.saved


def _run(form, index, shape, mode, bias, act, pipe=None):
    """(output tensor, fp64 reference) of candidate `index` under a call form."""
    host, dev, ref = _case(shape)
    s13 = R.shape13(shape)
    conv = T.with_bias(ref[mode], host["b"]) if bias else ref[mode]
    bd = dev["b"] if bias else None
    with _env(pipe):
        if form == "plain":
            return T.run_plan(index, dev["x"], dev["w"], bd, s13, None, mode), conv
        rd, rh = (dev["res"], host["res"]) if form == "res" else (None, None)
        y = T.run_fused(index, dev["x"], dev["w"], bd, s13, None, mode, post_scale=dev["ps"], post_shift=dev["pb"],
                        residual=rd, act=act)
    return y, T.epilogue(conv, host["ps"], host["pb"], rh, act)


def _check_row(n, r):
    bias, act = n % 3 != 0, ACTS[n % 4]
    for mode in MODES:
        found = R.find_plan(r, mode)
        assert found is not None, (R.row_id(r), mode)
        index, p = found
        sib = [(sel, R.find_plan(r, mode, sel)) for sel in R.siblings(r)]
        for form in r.forms:
            if form in ("ds", "ds_epi"):
                _check_ds(r, form, mode, act)
                continue
            outs = {}
            for pipe in (r.pipes if form in ("plain", "epi") else (None,)):
                y, ref = _run(form, index, r.shape, mode, bias, act, pipe)
                err = normwise_err(y.cpu().numpy(), ref)
                print("%s %s %s pipe=%s %s err=%.3g" % (R.row_id(r), mode, form, pipe, R.dispatch(p, r.shape, form, pipe), err))
                assert err <= CONV_TOL, (R.row_id(r), mode, form, pipe, err)
                outs[pipe] = y
            # bit-for-bit siblings: PIPE on / off, nts = 0, fp = 0 change no summation order
            first = outs[r.pipes[0] if form in ("plain", "epi") else None]
            for pipe, y in outs.items():
                assert torch.equal(y, first), (R.row_id(r), mode, form, "PIPE", pipe)
            for sel, f in sib:
                assert f is not None, (R.row_id(r), mode, sel)
                ys, _ = _run(form, f[0], r.shape, mode, bias, act)
                assert torch.equal(ys, first), (R.row_id(r), mode, form, "sibling", sel)


def _check_ds(r, form, mode, act):
    """po2q_qconv2d_s2ds_f32 (the plan s2ds_plan picks: the row's, test_rows_cases_cpu.py): conv and shortcut."""
    host, dev, ref = _case(r.shape)
    wds, refd = _case_ds(r.shape, mode)
    kw, ref3 = {}, ref[mode]
    if form == "ds_epi":
        kw = dict(post_scale=dev["ps"], post_shift=dev["pb"], act=act, post_scale_ds=dev["pb"] + 1.0, post_shift_ds=dev["ps"])
        ref3 = T.epilogue(ref3, host["ps"], host["pb"], None, act)
        refd = T.epilogue(refd, host["pb"] + 1.0, host["ps"])
    y, yd = _lib.qconv2d_s2ds(dev["x"], dev["w"], wds.to(DEV), 4, mode, **kw)
    for got, want, what in ((y, ref3, "conv"), (yd, refd, "shortcut")):
        err = normwise_err(got.cpu().numpy(), want)
        assert err <= CONV_TOL, (R.row_id(r), mode, form, what, err)


CHUNKS = [list(enumerate(R.ROWS))[i:i + CHUNK] for i in range(0, len(R.ROWS), CHUNK)]


@pytest.mark.parametrize("rows", CHUNKS, ids=["rows-%03d" % (i * CHUNK) for i in range(len(CHUNKS))])
def test_row_kernel_rows_vs_oracle(rows):
    for n, r in rows:
        _check_row(n, r)


GUARD_ROWS = [(n, r) for n, r in enumerate(R.ROWS) if any(c in R.GUARD_CONDS for c in r.conds)]
GUARD_CHUNKS = [GUARD_ROWS[i:i + 2 * CHUNK] for i in range(0, len(GUARD_ROWS), 2 * CHUNK)]


@pytest.mark.parametrize("rows", GUARD_CHUNKS, ids=["guard-%02d" % i for i in range(len(GUARD_CHUNKS))])
def test_no_store_outside_y(rows):
    """Ragged strips store float4s, short last segments and idle blocks walk past the image: y sits 16-byte aligned
    inside a sentinel-filled buffer with 4 KiB on either side, which must come back bit-unchanged."""
    for n, r in rows:
        host, dev, ref = _case(r.shape)
        N, C, H, W, K, st = r.shape
        P, Q = R.out_size(r.shape)
        ny = N * K * P * Q
        pad = -ny % 4      # keep the rear guard 16-byte aligned too
        for mode in MODES:
            index, _ = R.find_plan(r, mode)
            buf = torch.full((GUARD + ny + pad + GUARD,), SENTINEL, device=DEV)
            y = buf[GUARD:GUARD + ny].view(N, K, P, Q)
            assert y.data_ptr() % 16 == 0
            with _env(r.pipes[0]):
                T.run_plan(index, dev["x"], dev["w"], dev["b"], R.shape13(r.shape), None, mode, y=y)
            torch.cuda.synchronize()
            guard = torch.full((GUARD,), SENTINEL)
            assert torch.equal(buf[:GUARD].cpu(), guard), (R.row_id(r), mode, "a store landed before y")
            assert torch.equal(buf[GUARD + ny:].cpu(), torch.full((GUARD + pad,), SENTINEL)), (R.row_id(r), mode, "a store landed after y")
            err = normwise_err(y.cpu().numpy(), T.with_bias(ref[mode], host["b"]))
            assert err <= CONV_TOL, (R.row_id(r), mode, err)


@pytest.mark.parametrize("shape", [s for s, _ in R.FALLBACK_SHAPES], ids=lambda s: "x".join(map(str, s)))
def test_too_short_for_a_row_kernel_falls_to_another(shape):
    host, dev, ref = _case(shape)
    for mode in MODES:
        y = T.run_plan(0, dev["x"], dev["w"], dev["b"], R.shape13(shape), None, mode)
        err = normwise_err(y.cpu().numpy(), T.with_bias(ref[mode], host["b"]))
        assert err <= CONV_TOL, (shape, mode, err)


RES_OFF_ROWS = [n for n, r in enumerate(R.ROWS) if r.res_off]


def _res_off_child():
    """Runs in a fresh process under PO2Q_ROWSK_RES=0 (the switch is read once per process): the C = 64 rows'
    residual form, now the affine in the kernel and the residual as an elementwise pass."""
    out = []
    for n in RES_OFF_ROWS:
        r = R.ROWS[n]
        for mode in MODES:
            index, _ = R.find_plan(r, mode)
            y, ref = _run("res", index, r.shape, mode, True, "relu")
            out.append([R.row_id(r), mode, normwise_err(y.cpu().numpy(), ref)])
    print("RES_OFF " + json.dumps(out))


def test_c64_residual_with_the_in_kernel_switch_off():
    assert RES_OFF_ROWS
    env = dict(os.environ, PO2Q_ROWSK_RES="0")
    env.pop("PO2Q_ROWSK_PIPE", None)
    code = "from tests import test_gpu_rows_paths as t; t._res_off_child()"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cp = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr[-2000:]
    line = [ln for ln in cp.stdout.splitlines() if ln.startswith("RES_OFF ")][-1]
    got = json.loads(line[len("RES_OFF "):])
    assert len(got) == len(RES_OFF_ROWS) * len(MODES)
    for rid, mode, err in got:
        assert err <= CONV_TOL, (rid, mode, err)
    # and in this process, with the switch unset, the same calls take the in-kernel path at the same bar
    for n in RES_OFF_ROWS:
        r = R.ROWS[n]
        index, p = R.find_plan(r)
        assert R.res_in_kernel(p, r.shape)
        y, ref = _run("res", index, r.shape, "po2", True, "relu")
        assert normwise_err(y.cpu().numpy(), ref) <= CONV_TOL
