"""A/B of one transformer layer's MLP half on one token tensor: the fused kernel (torch.ops.po2q.ffn, po2q_ffn_f32)
forced to the token-tile kernel, forced to the hidden-split kernel and on auto, against the torch op sequence
Transformer.forward runs for x + ff(x) (models/mobile_vit.py): LayerNorm, Linear, SiLU, Linear, add.  GPU only.

    python tools/ffn_bench.py [--shapes 65536x96x192 16384x120x480 4096x144x576 --iters 50 --runs 5
                               --out profiles/ffn_ab.jsonl]

Defaults: config 5's three transformer stages at batch 64 (MobileViT-XS @256: M x dim x hidden).  All arms run in one
process on the same tensors, warmed up, in alternating runs of `iters` calls timed with device events; per arm the
median over the runs and their min / max are reported, one JSON line per shape, with each arm's normwise difference
against an fp64 evaluation of the first 256 tokens.
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


def torch_ffn(x, ln_w, ln_b, w1, b1, w2, b2):
    return x + F.linear(F.silu(F.linear(F.layer_norm(x, x.shape[-1:], ln_w, ln_b, EPS), w1, b1)), w2, b2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65536x96x192", "16384x120x480", "4096x144x576"],
                    help="M x dim x hidden")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops = _lib.ops()
    for shape in args.shapes:
        M, dim, hidden = (int(v) for v in shape.split("x"))
        torch.manual_seed(M + dim)
        x = torch.randn(M // 4, 4, dim, device=dev)
        ln_w, ln_b = 1 + 0.5 * torch.randn(dim, device=dev), 0.5 * torch.randn(dim, device=dev)
        w1, b1 = torch.randn(hidden, dim, device=dev) / dim ** 0.5, torch.randn(hidden, device=dev)
        w2, b2 = torch.randn(dim, hidden, device=dev) / hidden ** 0.5, torch.randn(dim, device=dev)
        p = (ln_w, ln_b, w1, b1, w2, b2)
        arms = {"torch": lambda: torch_ffn(x, *p)}
        for name, kernel in (("token_tiles", 1), ("hidden_split", 2), ("auto", 0)):
            arms[name] = lambda kernel=kernel: ops.ffn(x, ln_w, ln_b, EPS, w1, b1, w2, b2, True, kernel)
        res = {"kind": "ffn_ab", "M": M, "dim": dim, "hidden": hidden, "iters": args.iters, "runs": args.runs}
        res.update(_ab.ab(arms, lambda: torch_ffn(x[:64].double().cpu(), *(t.double().cpu() for t in p)),
                          lambda y: y[:64], args.iters, args.runs))
        res["speedup_auto"] = round(res["torch_us"] / res["auto_us"], 2)
        _ab.emit(res, args.out)


if __name__ == "__main__":
    main()
