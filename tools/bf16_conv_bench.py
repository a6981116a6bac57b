"""The bf16 conv entry against the fp32 entry on the ResNet56 @224, batch 256 layer shapes, same process,
same GPU, calls alternated:

    python tools/bf16_conv_bench.py [--out profiles/bf16_conv.jsonl --reps 40 --warmup 10 --batch 256]

  fp32   _lib.qconv2d(mode="po2") on fp32 tensors, its autotuned plan (bf16x3 kernels)
  bf16   _lib.qconv2d_bf16(mode="po2") on the same values in bf16 (heuristic tile, no autotuning)
Each call is the whole entry as a model forward issues it (weight quantize + pack launches and the
conv), timed with HIP events call by call after a warm-up; the two arms alternate inside one loop so
drift hits both.  One JSON line per shape: median and minimum microseconds of each arm, the
algorithmic bytes (x + y + w once, in the arm's dtype) and their fraction of the 8 TB/s HBM roof at
the median, and the fp32 / bf16 time ratio (> 1: bf16 faster).

    python tools/bf16_conv_bench.py --fused [--out profiles/bf16_fused.jsonl]

The fused bf16 epilogue: the same five layers with a bf16 eval BatchNorm + ReLU after the conv, then once
more with a residual of the output's shape added before the ReLU; three arms alternated call by call
(in the orders sequence, fused, plain and sequence, plain, fused in turn):
  sequence  _lib.qconv2d_bf16, then torch's BatchNorm, add and ReLU (the module sequence of a bf16 model)
  fused     _lib.qconv2d_fused_bf16 with the BatchNorm folded in fp32 (one launch for all of it)
  plain     the bare _lib.qconv2d_bf16 call, for reference
One JSON line per (layer, residual): the arms' median / minimum microseconds, the algorithmic bytes of the
fused call (x + y + w, plus the residual, in bf16) and their fraction of the HBM roof at each arm's median.

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from po2_quantization_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8e12  # MI355X peak HBM bandwidth

# (C, H, K, stride): 3x3, pad 1 -- the three stages' stride-1 layers and the two stride-2 transitions
SHAPES = [(16, 224, 16, 1), (32, 112, 32, 1), (64, 56, 64, 1), (16, 224, 32, 2), (32, 112, 64, 2)]


def algorithmic_bytes(N, C, H, K, stride, itemsize):
    P = (H + 2 - 3) // stride + 1
    return itemsize * (N * C * H * H + N * K * P * P + K * C * 9)


def time_arms(arms, warmup, reps):
    """Microseconds of each call of each arm, the arms alternated inside one loop.  With three arms the
    order alternates between (a, b, c) and (a, c, b), so b and c each follow a in half of their calls and
    each other in the other half: what the previous call left in the 256 MiB last-level cache (x is read by
    every arm) then favours neither."""
    ts = {k: [] for k in arms}
    names = list(arms)
    with torch.no_grad():
        for _ in range(warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        for rep in range(reps):
            for name in (names if rep % 2 == 0 else names[:1] + names[:0:-1]):
                fn = arms[name]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
    return ts


def fused_lines(a, dev):
    from po2_quantization_amd.models.quantized_conv import _torch_epilogue, fold_bn_f32

    N = a.batch
    lines = []
    for with_res in (False, True):
        for C, H, K, stride in SHAPES:
            torch.manual_seed(0)
            x = torch.randn(N, C, H, H, device=dev).to(torch.bfloat16)
            w = (torch.randn(K, C, 3, 3, device=dev) * 0.1).to(torch.bfloat16)
            bn = torch.nn.BatchNorm2d(K)
            with torch.no_grad():
                bn.running_mean.normal_()
                bn.running_var.uniform_(0.5, 2.0)
                bn.weight.normal_()
                bn.bias.normal_()
            bn = bn.bfloat16().to(dev).eval()
            ps, pb = fold_bn_f32(bn)
            P = (H + 2 - 3) // stride + 1
            res = torch.randn(N, K, P, P, device=dev).to(torch.bfloat16) if with_res else None

            def plain():
                return _lib.qconv2d_bf16(x, w, None, stride, 1, 1, 1, a.bits, "po2")

            arms = {
                "sequence": lambda: _torch_epilogue(plain(), bn, "relu", res),
                "fused": lambda: _lib.qconv2d_fused_bf16(x, w, None, stride, 1, 1, 1, a.bits, "po2", 1, post_scale=ps,
                                                         post_shift=pb, residual=res, act="relu"),
                "plain": plain,
            }
            ts = time_arms(arms, a.warmup, a.reps)
            nbytes = algorithmic_bytes(N, C, H, K, stride, 2) + (2 * N * K * P * P if with_res else 0)
            out = {"shape": [N, C, H, H, K, 3], "stride": stride, "pad": 1, "bits": a.bits, "mode": "po2",
                   "reps": a.reps, "epilogue": "bn+add+relu" if with_res else "bn+relu", "fused_bytes": nbytes}
            for name in arms:
                med = statistics.median(ts[name])
                out[name + "_us_median"] = round(med, 1)
                out[name + "_us_min"] = round(min(ts[name]), 1)
                out[name + "_roof_fraction_of_fused_bytes"] = round(nbytes / HBM_BYTES_PER_S / (med * 1e-6), 3)
            out["sequence_over_fused_time"] = round(out["sequence_us_median"] / out["fused_us_median"], 3)
            out["fused_over_plain_time"] = round(out["fused_us_median"] / out["plain_us_median"], 3)
            out["bf16_plan"] = _lib.describe_bf16(N, C, H, H, K, 3, 3, stride, 1, 1, 1, a.bits, "po2")
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            del x, w, res
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused", action="store_true", help="time the fused bf16 epilogue against the module sequence")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bits", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_conv_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bf16_fused.jsonl" if a.fused else "bf16_conv.jsonl")
    if a.fused:
        lines = fused_lines(a, dev)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    _lib.benchmark = True  # the fp32 entry autotunes on its first call
    N = a.batch
    lines = []
    for C, H, K, stride in SHAPES:
        torch.manual_seed(0)
        x32 = torch.randn(N, C, H, H, device=dev)
        w32 = torch.randn(K, C, 3, 3, device=dev) * 0.1
        x16, w16 = x32.to(torch.bfloat16), w32.to(torch.bfloat16)
        arms = {
            "fp32": lambda: _lib.qconv2d(x32, w32, None, stride, 1, 1, 1, a.bits, "po2"),
            "bf16": lambda: _lib.qconv2d_bf16(x16, w16, None, stride, 1, 1, 1, a.bits, "po2"),
        }
        ts = time_arms(arms, a.warmup, a.reps)
        res = {"shape": [N, C, H, H, K, 3], "stride": stride, "pad": 1, "bits": a.bits, "mode": "po2", "reps": a.reps}
        for name, itemsize in (("fp32", 4), ("bf16", 2)):
            med = statistics.median(ts[name])
            nbytes = algorithmic_bytes(N, C, H, K, stride, itemsize)
            res[name + "_us_median"] = round(med, 1)
            res[name + "_us_min"] = round(min(ts[name]), 1)
            res[name + "_bytes"] = nbytes
            res[name + "_hbm_roof_fraction"] = round(nbytes / HBM_BYTES_PER_S / (med * 1e-6), 3)
        res["fp32_over_bf16_time"] = round(res["fp32_us_median"] / res["bf16_us_median"], 3)
        res["fp32_plan"] = _lib.describe(N, C, H, H, K, 3, 3, stride, 1, 1, 1, a.bits, "po2")
        res["bf16_plan"] = _lib.describe_bf16(N, C, H, H, K, 3, 3, stride, 1, 1, 1, a.bits, "po2")
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del x32, w32, x16, w16
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
