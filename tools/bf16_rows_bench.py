"""The bf16 row-streaming conv kernels against the bf16 tile kernel and the fp32 entry on the layer classes
they were written for (ResNet56 @224, batch 256: 16 -> 16 @224, 32 -> 32 @112 and 64 -> 64 @56, 3x3, pad 1):

    python tools/bf16_rows_bench.py [--out profiles/bf16_rows.jsonl --reps 40 --warmup 10 --batch 256 --runs 2]
    python tools/bf16_rows_bench.py --layers 64@56,64@28,64@14,64@8 --out profiles/bf16_rowsk.jsonl

Three arms, alternated call by call in one process (time_arms of tools/bf16_conv_bench.py), HIP events
around each whole call (weight quantize + pack launches and the conv, as a model forward issues them):
  fp32   _lib.qconv2d / _lib.qconv2d_fused on fp32 tensors, the autotuned plan
  tile   _lib.qconv2d_bf16 / _lib.qconv2d_fused_bf16 with both row-kernel switches off (conv_bf16x1)
  rows   the same call with _lib.set_bf16_row_kernels(True) and _lib.set_bf16_rowsk_kernels(True)
         (conv_b16_rows at C = 16 / 32, conv_b16_rowsk at C = 64)
Three forms per layer: the plain conv, the conv with a folded eval BatchNorm + ReLU in its store, and the
same with a residual added before the ReLU.  Every (layer, form) is timed --runs times; one JSON line per
(layer, form) with each run's median and minimum microseconds per arm, the spread (the largest difference
between two runs' medians of one arm), the bf16 bytes' fraction of the 8 TB/s HBM roof at the row arm's
median, and whether the row arm's worst median is below the tile arm's best by more than the spread.

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_conv_bench import HBM_BYTES_PER_S, algorithmic_bytes, time_arms  # noqa: E402
from po2_quantization_amd import _lib  # noqa: E402
from po2_quantization_amd.models.quantized_conv import fold_bn_f32  # noqa: E402

LAYERS = "16@224,32@112"  # C = K @ H = W; --layers 64@56 for stage 3
FORMS = ["plain", "bn+relu", "bn+add+relu"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_rows.jsonl"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--layers", default=LAYERS, help="comma-separated C@H layers (C = K, H = W)")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in item.split("@")) for item in a.layers.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("bf16_rows_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    _lib.benchmark = True  # the fp32 entry autotunes on its first call
    N = a.batch
    lines = []
    for C, H in shapes:
        torch.manual_seed(0)
        x32 = torch.randn(N, C, H, H, device=dev)
        w32 = torch.randn(C, C, 3, 3, device=dev) * 0.1
        x16, w16 = x32.to(torch.bfloat16), w32.to(torch.bfloat16)
        bn = torch.nn.BatchNorm2d(C)
        with torch.no_grad():
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
            bn.weight.normal_()
            bn.bias.normal_()
        ps, pb = fold_bn_f32(bn.to(dev).eval())
        r32 = torch.randn(N, C, H, H, device=dev)
        r16 = r32.to(torch.bfloat16)
        with _lib.bf16_rows(False), _lib.bf16_rowsk(False):
            tile_plan = _lib.describe_bf16(N, C, H, H, C, 3, 3, 1, 1, 1, 1, a.bits, "po2")
        with _lib.bf16_rows(True), _lib.bf16_rowsk(True):
            rows_plan = _lib.describe_bf16(N, C, H, H, C, 3, 3, 1, 1, 1, 1, a.bits, "po2")
        for form in FORMS:
            res32, res16 = (r32, r16) if form == "bn+add+relu" else (None, None)

            def fp32():
                if form == "plain":
                    return _lib.qconv2d(x32, w32, None, 1, 1, 1, 1, a.bits, "po2")
                return _lib.qconv2d_fused(x32, w32, None, 1, 1, 1, 1, a.bits, "po2", post_scale=ps, post_shift=pb,
                                          residual=res32, act="relu")

            def bf16():
                if form == "plain":
                    return _lib.qconv2d_bf16(x16, w16, None, 1, 1, 1, 1, a.bits, "po2")
                return _lib.qconv2d_fused_bf16(x16, w16, None, 1, 1, 1, 1, a.bits, "po2", 1, post_scale=ps,
                                               post_shift=pb, residual=res16, act="relu")

            def tile():
                with _lib.bf16_rows(False), _lib.bf16_rowsk(False):
                    return bf16()

            def rows():
                with _lib.bf16_rows(True), _lib.bf16_rowsk(True):
                    return bf16()

            arms = {"fp32": fp32, "tile": tile, "rows": rows}
            runs = [time_arms(arms, a.warmup, a.reps) for _ in range(a.runs)]
            nbytes = algorithmic_bytes(N, C, H, C, 1, 2) + (2 * N * C * H * H if res16 is not None else 0)
            out = {"shape": [N, C, H, H, C, 3], "stride": 1, "pad": 1, "bits": a.bits, "mode": "po2", "form": form,
                   "reps": a.reps, "runs": a.runs, "bf16_bytes": nbytes}
            spread = 0.0
            for name in arms:
                meds = [round(statistics.median(ts[name]), 1) for ts in runs]
                out[name + "_us_median"] = meds
                out[name + "_us_min"] = [round(min(ts[name]), 1) for ts in runs]
                spread = max(spread, max(meds) - min(meds))
            out["spread_us"] = round(spread, 1)
            out["rows_hbm_roof_fraction"] = round(nbytes / HBM_BYTES_PER_S / (max(out["rows_us_median"]) * 1e-6), 3)
            out["tile_over_rows_time"] = round(min(out["tile_us_median"]) / max(out["rows_us_median"]), 3)
            out["fp32_over_rows_time"] = round(min(out["fp32_us_median"]) / max(out["rows_us_median"]), 3)
            out["rows_beats_tile_by_more_than_spread"] = bool(
                min(out["tile_us_median"]) - max(out["rows_us_median"]) > spread)
            out["tile_plan"], out["rows_plan"] = tile_plan, rows_plan
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
        del x32, w32, x16, w16, r32, r16
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
