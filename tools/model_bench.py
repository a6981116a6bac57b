"""Model-level inference throughput (images/s) of the reference's model graphs on the
drop-in modules, with and without the fused conv epilogue:

    python tools/model_bench.py [--model resnet56 --image 224 --batch 256 --classes 1000]

Synthetic NCHW input, random-init weights (seeded), eval mode, torch.no_grad().
"fused": conv+BN(+add)+act as one native call per conv; "unfused": the reference's
module sequence (native conv, torch BatchNorm / ReLU / add).  GPU only.

    python tools/model_bench.py --dtype bf16 [--bf16-row-kernels --bf16-rowsk-kernels --bf16-fused-epilogue]
                                [--steps 20 --warmup 5 --runs 2]

The bf16 forward (model.bfloat16(), bf16 input) in four arms: both row-kernel switches off, the first on,
both on, both on with the fused epilogue (models.quantized_conv.BF16_FUSED_EPILOGUE).  The arms named by
the flags are timed (no flag: all four), alternated forward by forward in one process with HIP events
around each whole forward; one JSON line with every run's median milliseconds per arm and the spread
between runs."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from po2_quantization_amd import _lib  # noqa: E402
from po2_quantization_amd.models import quantized_conv  # noqa: E402
from po2_quantization_amd.models.model import get_model  # noqa: E402
from po2_quantization_amd.utils.quantizers import quantizer_dict  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


BF16_ARMS = {  # name -> (first switch, C = 64 switch, fused epilogue)
    "off": (False, False, False),
    "rows": (True, False, False),
    "rows+rowsk": (True, True, False),
    "rows+rowsk+fused": (True, True, True),
}


def bf16_arms(args):
    """The arms the flags name, beside the both-off arm; no flag: all four."""
    if not (args.bf16_row_kernels or args.bf16_rowsk_kernels or args.bf16_fused_epilogue):
        return dict(BF16_ARMS)
    name = "+".join(n for n, on in (("rows", args.bf16_row_kernels), ("rowsk", args.bf16_rowsk_kernels),
                                    ("fused", args.bf16_fused_epilogue)) if on)
    return {"off": BF16_ARMS["off"],
            name: (args.bf16_row_kernels, args.bf16_rowsk_kernels, args.bf16_fused_epilogue)}


def bench_bf16(args):
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    m = get_model(args.model, args.classes, quantizer_dict[args.quantizer], args.bits,
                  (args.image, args.image)).to(dev).eval().bfloat16()
    x = torch.randn(args.batch, 3, args.image, args.image, device=dev).to(torch.bfloat16)
    arms = bf16_arms(args)
    saved = quantized_conv.BF16_FUSED_EPILOGUE

    def forward(setting):
        first, new, fused = setting
        quantized_conv.BF16_FUSED_EPILOGUE = fused
        with _lib.bf16_rows(first), _lib.bf16_rowsk(new):
            return m(x)

    res = {"model": args.model, "image": args.image, "batch": args.batch, "quantizer": args.quantizer,
           "bits": args.bits, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "runs": args.runs}
    try:
        with torch.no_grad():
            meds = {name: [] for name in arms}
            for _ in range(args.runs):
                ev = {name: [] for name in arms}
                for i in range(args.warmup + args.steps):
                    for name, setting in arms.items():  # alternated forward by forward
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        forward(setting)
                        e1.record()
                        if i >= args.warmup:
                            ev[name].append((e0, e1))
                torch.cuda.synchronize()
                for name in arms:
                    meds[name].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[name]))
            off = forward(arms["off"]).float()
            for name, setting in arms.items():
                res[name + "_ms_median"] = [round(v, 3) for v in meds[name]]
                res[name + "_images_per_s"] = round(args.batch / (max(meds[name]) * 1e-3), 1)
                res[name + "_logits_vs_off_normwise"] = float((forward(setting).float() - off).abs().max() / off.abs().max())
            res["spread_ms"] = round(max(max(v) - min(v) for v in meds.values()), 3)
    finally:
        quantized_conv.BF16_FUSED_EPILOGUE = saved
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet56")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--quantizer", default="po2")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--graph", action="store_true",
                    help="also time the fused forward replayed from a HIP graph (small images: launch-bound)")
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--no-ir", action="store_true",
                    help="inverted-residual blocks as three fused layer calls instead of one block launch")
    ap.add_argument("--ir", action="store_true", help="inverted-residual blocks as one launch where it applies")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--bf16-row-kernels", action="store_true", help="with --dtype bf16: time the arm with the C = 16 / 32 row kernel")
    ap.add_argument("--bf16-rowsk-kernels", action="store_true", help="with --dtype bf16: ... with the C = 64 row kernel")
    ap.add_argument("--bf16-fused-epilogue", action="store_true", help="with --dtype bf16: ... with the fused epilogue")
    ap.add_argument("--runs", type=int, default=2, help="with --dtype bf16: timed runs (the spread is between their medians)")
    args = ap.parse_args()
    if args.dtype == "bf16":
        return bench_bf16(args)
    if args.bf16_row_kernels or args.bf16_rowsk_kernels or args.bf16_fused_epilogue:
        ap.error("the --bf16-* options need --dtype bf16")
    if args.ir or args.no_ir:
        quantized_conv.IR_FUSION = bool(args.ir)
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    m = get_model(args.model, args.classes, quantizer_dict[args.quantizer], args.bits,
                  (args.image, args.image)).to(dev).eval()
    x = torch.randn(args.batch, 3, args.image, args.image, device=dev)
    _lib.benchmark = True  # autotune every conv shape once (cudnn.benchmark counterpart)
    res = {"model": args.model, "image": args.image, "batch": args.batch, "quantizer": args.quantizer,
           "bits": args.bits, "ir_fusion": quantized_conv.IR_FUSION}
    with torch.no_grad():
        for name, fuse in (("fused", True), ("unfused", False)):
            if args.only_fused and not fuse:
                continue
            quantized_conv.INFERENCE_FUSION = fuse
            t = timed(lambda: m(x), args.steps, args.warmup)
            res[name + "_ms"] = round(t * 1e3, 3)
            res[name + "_images_per_s"] = round(args.batch / t, 1)
        if args.graph:
            quantized_conv.INFERENCE_FUSION = True
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                m(x)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                m(x)
            t = timed(g.replay, args.steps * 4, args.warmup)
            res["graph_fused_ms"] = round(t * 1e3, 3)
            res["graph_fused_images_per_s"] = round(args.batch / t, 1)
        if not args.only_fused:
            quantized_conv.INFERENCE_FUSION = True
            ya = m(x)
            quantized_conv.INFERENCE_FUSION = False
            yb = m(x)
            quantized_conv.INFERENCE_FUSION = True
            res["fused_vs_unfused_normwise"] = float((ya - yb).abs().max() / yb.abs().max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
