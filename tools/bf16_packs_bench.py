"""Batched weight packs of the bf16 forward (models/quantized_conv.py BATCHED_PACKS on a bf16 input) against
the per-layer staging, whole eval forwards at batch 256, same process, same GPU:

    python tools/bf16_packs_bench.py [--out profiles/bf16_packs.jsonl --reps 40 --warmup 10 --batch 256]

  off   every conv stages its own weight: max|w|, quantize + pack, conv (po2q_qconv2d_bf16; the path before
        the batched packs existed, bit for bit)
  on    the recorded layers' staging as one pack_batch_bf16 call up front, each conv from its pack
Configs: ResNet56 @32 and MobileNetV2 @32 (launch-bound), ResNet56 @224 (where the packs should not matter).
The arms alternate forward by forward and swap their order between rounds; HIP events surround each
forward.  Each config is timed twice: eager, and replayed from one HIP graph per arm, where the host's
launch latency is gone and only the device's own time differs.  The logits of the two arms are compared
(they must be equal) before anything is timed.

One JSON line per (config, eager | graph): median and minimum microseconds of each arm, on / off, and the
conv-side launches per forward of each arm, counted from the calls the forward makes (not estimated):
a call of the unbatched entry is its conv plus two staging launches (one in mode none), a packed call
is one, and a pack_batch_bf16 call of n layers is, per group of 36, one quantize + pack launch plus one
max|w| launch when the group has a quantized layer (include/po2q.h).

    python tools/bf16_packs_bench.py --off-only --tag parent --append

times the eager off arm alone.  Copied into a built checkout of the commit before the batched entries and
run there, in the same job on the same GPU, it is the check that the unbatched entry did not move.

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
from po2_quantization_amd.models import quantized_conv as qc  # noqa: E402
from po2_quantization_amd.models.model import get_model  # noqa: E402
from po2_quantization_amd.utils.quantizers import quantizer_dict  # noqa: E402

CONFIGS = [("resnet56", 32), ("mobilenet", 32), ("resnet56", 224)]
GROUP = 36  # jobs per launch of po2q_qconv2d_bf16_pack_batch


def forward(model, x, packs):
    qc.BATCHED_PACKS = packs
    with torch.no_grad():
        return model(x)


def count_launches(model, x, packs):
    """Conv-side launches of one forward, from the calls it makes."""
    n = {"launches": 0, "convs": 0}
    real = {k: getattr(_lib, k) for k in ("qconv2d_bf16", "qconv2d_fused_bf16", "qconv2d_packed_bf16", "pack_batch_bf16")}

    def own(fn, mode_at):
        def f(*a, **k):
            mode = k.get("mode", a[mode_at] if len(a) > mode_at else "po2")
            n["launches"] += 2 if mode in (None, "none") else 3
            n["convs"] += 1
            return fn(*a, **k)
        return f

    def packed(*a, **k):
        n["launches"] += 1
        n["convs"] += 1
        return real["qconv2d_packed_bf16"](*a, **k)

    def batch(layers, bits=4, mode="po2", fsr=1):
        modes = list(mode) if isinstance(mode, (list, tuple)) else [mode] * len(layers)
        for i in range(0, len(layers), GROUP):
            n["launches"] += 1 + any(m not in (None, "none") for m in modes[i:i + GROUP])
        return real["pack_batch_bf16"](layers, bits, mode, fsr)

    _lib.qconv2d_bf16, _lib.qconv2d_fused_bf16 = own(real["qconv2d_bf16"], 8), own(real["qconv2d_fused_bf16"], 8)
    _lib.qconv2d_packed_bf16, _lib.pack_batch_bf16 = packed, batch
    try:
        forward(model, x, packs)
    finally:
        for k, fn in real.items():
            setattr(_lib, k, fn)
    return n


def time_arms(arms, warmup, reps):
    """Microseconds of each call of each arm; the arms alternate call by call, their order swaps every round."""
    ts = {k: [] for k in arms}
    names = list(arms)
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    for rep in range(reps):
        for name in (names if rep % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            arms[name]()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    return ts


def capture(model, x, packs):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        forward(model, x, packs)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = forward(model, x, packs)
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_packs.jsonl"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--fused-epilogue", action="store_true", help="BF16_FUSED_EPILOGUE on (default: the module sequence)")
    ap.add_argument("--off-only", action="store_true", help="the eager off arm alone (a library without the batch entries)")
    ap.add_argument("--tag", default="this", help="names the library build in the output lines")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_packs_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    qc.BF16_FUSED_EPILOGUE = a.fused_epilogue
    lines = []
    for name, image in CONFIGS:
        torch.manual_seed(0)
        model = get_model(name, 10, quantizer_dict["po2"], a.bits, (image, image)).eval().bfloat16().to(dev)
        x = torch.randn(a.batch, 3, image, image, device=dev).to(torch.bfloat16)
        base = {"model": name, "image": image, "batch": a.batch, "bits": a.bits, "mode": "po2", "reps": a.reps,
                "fused_epilogue": a.fused_epilogue, "library": a.tag}
        if a.off_only:
            runs = [("eager", {"off": lambda: forward(model, x, False)}, None)]
        else:
            ref = forward(model, x, False)
            forward(model, x, True)  # records the layers
            assert torch.equal(forward(model, x, True), ref), "the batched packs changed the logits"
            counts = {"off": count_launches(model, x, False), "on": count_launches(model, x, True)}
            g_off, o_off = capture(model, x, False)
            g_on, o_on = capture(model, x, True)
            g_off.replay(), g_on.replay()
            torch.cuda.synchronize()
            assert torch.equal(o_off, ref) and torch.equal(o_on, ref), "a graph replay changed the logits"
            runs = [("eager", {"off": lambda: forward(model, x, False), "on": lambda: forward(model, x, True)}, counts),
                    ("graph", {"off": g_off.replay, "on": g_on.replay}, counts)]
        for how, arms, counts in runs:
            ts = time_arms(arms, a.warmup, a.reps)
            out = dict(base, run=how)
            for arm in arms:
                out[arm + "_us_median"] = round(statistics.median(ts[arm]), 1)
                out[arm + "_us_min"] = round(min(ts[arm]), 1)
                q = statistics.quantiles(ts[arm], n=4)
                out[arm + "_us_iqr"] = round(q[2] - q[0], 1)
                if counts is not None:
                    out[arm + "_conv_calls"] = counts[arm]["convs"]
                    out[arm + "_conv_side_launches"] = counts[arm]["launches"]
            if "on" in arms:
                out["on_over_off_median"] = round(out["on_us_median"] / out["off_us_median"], 4)
                out["on_over_off_min"] = round(out["on_us_min"] / out["off_us_min"], 4)
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
        del model, x, runs
        torch.cuda.empty_cache()
    qc.BATCHED_PACKS = True
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
