"""A/B of one attention layer's core on one qkv tensor: the fused kernel (torch.ops.po2q.mhsa, po2q_mhsa_f32) against
the torch op sequence Attention.forward runs between to_qkv and to_out (models/mobile_vit.py): chunk / transpose views,
q k^T, scale, softmax, p v, transpose + reshape copy.  GPU only.

    python tools/mhsa_bench.py [--seqs 256 --tokens 256 64 16 --iters 50 --runs 5 --out profiles/mhsa_ab.jsonl]

Defaults: config 5's three transformer stages at batch 64 (MobileViT-XS @256: 256 sequences of 256 / 64 / 16 tokens,
4 heads of 8).  Both arms run in one process on the same tensor, warmed up, in alternating runs of `iters` calls timed
with device events; per arm the median over the runs and their min / max are reported, one JSON line per token count,
with the two arms' normwise difference against an fp64 evaluation of 8 of the sequences.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _ab  # noqa: E402  (tools/_ab.py, next to this script)
from po2_quantization_amd import _lib  # noqa: E402

HEADS, DIM_HEAD = 4, 8
SCALE = DIM_HEAD ** -0.5


def torch_core(qkv):
    b, p, n, _ = qkv.shape
    q, k, v = (t.view(b, p, n, HEADS, -1).transpose(2, 3) for t in qkv.chunk(3, dim=-1))
    attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * SCALE, dim=-1)
    return torch.matmul(attn, v).transpose(2, 3).reshape(b, p, n, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--tokens", type=int, nargs="+", default=[256, 64, 16])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops = _lib.ops()
    for n in args.tokens:
        torch.manual_seed(n)
        qkv = torch.randn(args.seqs // 4, 4, n, 3 * HEADS * DIM_HEAD, device=dev)
        arms = {"torch": lambda: torch_core(qkv), "native": lambda: ops.mhsa(qkv, HEADS, SCALE)}
        res = {"kind": "mhsa_ab", "seqs": args.seqs, "tokens": n, "heads": HEADS, "dim_head": DIM_HEAD,
               "iters": args.iters, "runs": args.runs}
        res.update(_ab.ab(arms, lambda: torch_core(qkv[:2].double().cpu()), lambda y: y[:2], args.iters, args.runs))
        res["speedup"] = round(res["torch_us"] / res["native_us"], 2)
        _ab.emit(res, args.out)


if __name__ == "__main__":
    main()
