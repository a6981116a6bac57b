"""A/B of the two projections around one transformer layer's attention core on one token tensor: the fused kernel
(torch.ops.po2q.ln_linear, po2q_ln_linear_f32) forced to the weight-resident kernel, forced to the out-split kernel and
on auto, against the torch op sequence Attention.forward / Transformer.forward run (models/mobile_vit.py): layer_norm +
linear for to_qkv(norm(x)), linear + add for x + to_out(core).  GPU only.

    python tools/lnlin_bench.py [--shapes qkv:65536x96x96 out:65536x32x96 ... --iters 50 --runs 5
                                 --out profiles/lnlin_ab.jsonl]

Defaults: config 5's three transformer stages at batch 64 (MobileViT-XS @256), both halves (half:M x in x out).  All
arms run in one process on the same tensors, warmed up, in alternating runs of `iters` calls timed with device events;
per arm the median over the runs and their min / max are reported, one JSON line per shape, with each arm's normwise
difference against an fp64 evaluation of the first 256 tokens.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _ab  # noqa: E402  (tools/_ab.py, next to this script)
from po2_quantization_amd import _lib  # noqa: E402

EPS = 1e-5
DEFAULT = ["qkv:65536x96x96", "qkv:16384x120x96", "qkv:4096x144x96",
           "out:65536x32x96", "out:16384x32x120", "out:4096x32x144"]


def torch_qkv(x, ln_w, ln_b, w):
    return F.linear(F.layer_norm(x, x.shape[-1:], ln_w, ln_b, EPS), w)


def torch_out(x, w, bias, residual):
    return residual + F.linear(x, w, bias)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=DEFAULT, help="half:M x in_dim x out_dim, half in {qkv, out}")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops = _lib.ops()
    for shape in args.shapes:
        half, _, dims = shape.partition(":")
        M, in_dim, out_dim = (int(v) for v in dims.split("x"))
        torch.manual_seed(M + in_dim + out_dim)
        x = torch.randn(M // 4, 4, in_dim, device=dev)
        w = torch.randn(out_dim, in_dim, device=dev) / in_dim ** 0.5
        if half == "qkv":
            ln_w, ln_b = 1 + 0.5 * torch.randn(in_dim, device=dev), 0.5 * torch.randn(in_dim, device=dev)
            arms = {"torch": lambda: torch_qkv(x, ln_w, ln_b, w)}
            native = lambda kernel: ops.ln_linear(x, ln_w, ln_b, EPS, w, None, None, kernel)  # noqa: E731
            ref = lambda: torch_qkv(x[:64].double().cpu(), *(t.double().cpu() for t in (ln_w, ln_b, w)))  # noqa: E731
        else:
            bias, residual = torch.randn(out_dim, device=dev), torch.randn(M // 4, 4, out_dim, device=dev)
            arms = {"torch": lambda: torch_out(x, w, bias, residual)}
            native = lambda kernel: ops.ln_linear(x, None, None, EPS, w, bias, residual, kernel)  # noqa: E731
            ref = lambda: torch_out(x[:64].double().cpu(), w.double().cpu(), bias.double().cpu(),  # noqa: E731
                                    residual[:64].double().cpu())
        for name, kernel in (("resident", 1), ("out_split", 2), ("auto", 0)):
            arms[name] = lambda kernel=kernel: native(kernel)
        res = {"kind": "lnlin_ab", "half": half, "M": M, "in_dim": in_dim, "out_dim": out_dim, "iters": args.iters,
               "runs": args.runs}
        res.update(_ab.ab(arms, ref, lambda y: y[:64], args.iters, args.runs))
        res["speedup_auto"] = round(res["torch_us"] / res["auto_us"], 2)
        _ab.emit(res, args.out)


if __name__ == "__main__":
    main()
