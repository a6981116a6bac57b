"""One conv layer in the lin / lin+ conv modes against the quantize-then-conv route, timed with HIP events:

    python tools/lin_conv_bench.py [--shape 256,16,224,224,16,3 --stride 1 --pad 1 --bits 4 --quantizer lin]

  native   _lib.qconv2d(mode="lin"): per-channel step + pack + bf16x3 conv inside the library
  split    _lib.quantize_lin(w) then _lib.qconv2d(mode="none"): a quantizer launch + the fp32 kernels
           (the route of QuantizedConv2d with NATIVE_LIN = False)
  po2      _lib.qconv2d(mode="po2") of the same shape, for scale
Every arm is autotuned first, warmed up, then timed call by call; prints one JSON line with the
median and minimum in microseconds."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from po2_quantization_amd import _lib  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(ts), 1), round(min(ts), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="256,16,224,224,16,3", help="N,C,H,W,K,R")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--pad", type=int, default=1)
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--quantizer", default="lin", choices=["lin", "lin+"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    N, C, H, W, K, R = (int(v) for v in a.shape.split(","))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(N, C, H, W, device=dev)
    w = torch.randn(K, C // a.groups, R, R, device=dev) * 0.2
    _lib.benchmark = True
    plus = a.quantizer == "lin+"
    conv = lambda wt, mode, fsr: _lib.qconv2d(x, wt, None, a.stride, a.pad, 1, a.groups, a.bits, mode, fsr)  # noqa: E731
    arms = {
        "native": lambda: conv(w, a.quantizer, 10),
        "split": lambda: conv(_lib.quantize_lin(w, a.bits, plus, 10), "none", 1),
        "po2": lambda: conv(w, "po2", 1),
    }
    res = {"shape": [N, C, H, W, K, R], "stride": a.stride, "pad": a.pad, "groups": a.groups, "bits": a.bits,
           "quantizer": a.quantizer}
    with torch.no_grad():
        ya, yb = arms["native"](), arms["split"]()
        res["native_vs_split_normwise"] = float((ya - yb).abs().max() / yb.abs().max())
        for name, fn in arms.items():
            med, mn = timed(fn, a.reps, a.warmup)
            res[name + "_us_median"], res[name + "_us_min"] = med, mn
    res["native_plan"] = _lib.describe(N, C, H, W, K, R, R, a.stride, a.pad, 1, a.groups, a.bits, a.quantizer, 10)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
