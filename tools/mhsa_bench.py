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
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from po2_quantization_amd import _lib  # noqa: E402

HEADS, DIM_HEAD = 4, 8
SCALE = DIM_HEAD ** -0.5


def torch_core(qkv):
    b, p, n, _ = qkv.shape
    q, k, v = (t.view(b, p, n, HEADS, -1).transpose(2, 3) for t in qkv.chunk(3, dim=-1))
    attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * SCALE, dim=-1)
    return torch.matmul(attn, v).transpose(2, 3).reshape(b, p, n, -1)


def run_us(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


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
    lines = []
    for n in args.tokens:
        torch.manual_seed(n)
        qkv = torch.randn(args.seqs // 4, 4, n, 3 * HEADS * DIM_HEAD, device=dev)
        arms = {"torch": lambda: torch_core(qkv), "native": lambda: ops.mhsa(qkv, HEADS, SCALE)}
        with torch.no_grad():
            ref = torch_core(qkv[:2].double().cpu())
            res = {"kind": "mhsa_ab", "seqs": args.seqs, "tokens": n, "heads": HEADS, "dim_head": DIM_HEAD,
                   "iters": args.iters, "runs": args.runs}
            for name, fn in arms.items():
                res[name + "_vs_fp64_normwise"] = float((fn()[:2].cpu().double() - ref).abs().max() / ref.abs().max())
                run_us(fn, args.iters)  # warm-up
            times = {name: [] for name in arms}
            for _ in range(args.runs):
                for name, fn in arms.items():
                    times[name].append(run_us(fn, args.iters))
        for name, v in times.items():
            res[name + "_us"] = round(statistics.median(v), 2)
            res[name + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        res["speedup"] = round(res["torch_us"] / res["native_us"], 2)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
