"""Same-build A/B of the conv-1 waves' schedule in the role-split conv pairs, JSON lines on stdout.

  python tools/pair_pipe_ab.py [--rounds 5] [--only pair64]
      old schedule (the conv-1 waves' vector work in front of their MFMAs) against the pipelined one
      (the vector work in slices between the MFMAs), chosen per call through the kernel's knob:
        conv_pairw   (256, 32, 112, 112)  PO2Q_PAIR_W32_PIPE=0 / 1
        conv_pair64  (256, 64, 56, 56)    PO2Q_PAIR64_PIPE=0 / 1
      one qconv2d_pair call per timing (weight pack + pair kernel), HIP events, the median of 31 calls
      per timing, `rounds` interleaved rounds per arm after a warm-up of both arms (about a second: the
      first timings of a process otherwise fall with the clocks settling).  A kernel's new form counts
      as faster only if its median beats the old form's by more than the spread (max - min) of the old
      arm's rounds; the outputs of the two arms are compared bit for bit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {
    "pairw": {"shape": (256, 32, 112, 112), "knob": "PO2Q_PAIR_W32_PIPE"},
    "pair64": {"shape": (256, 64, 56, 56), "knob": "PO2Q_PAIR64_PIPE"},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, choices=sorted(KERNELS))
    args = ap.parse_args()

    import torch

    from po2_quantization_amd import _lib
    from tools.pair64_ab import scoped_env
    from tools.tile_sweep import timeit

    dev = torch.device("cuda:0")
    for name, k in KERNELS.items():
        if args.only and name != args.only:
            continue
        N, C, H, W = k["shape"]
        g = torch.Generator().manual_seed(0)
        x = torch.relu(torch.randn(N, C, H, W, generator=g)).to(dev)
        w1, w2 = ((torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5).to(dev) for _ in range(2))
        fn = lambda: _lib.qconv2d_pair(x, w1, w2, 4, "po2")  # noqa: E731
        ts, outs = {"old": [], "new": []}, {}
        for _ in range(20):  # warm-up, both arms
            for v in ("0", "1"):
                with scoped_env({k["knob"]: v}):
                    timeit(fn, 61)
        for r in range(args.rounds):
            for arm in (("old", "new") if r % 2 == 0 else ("new", "old")):
                with scoped_env({k["knob"]: "0" if arm == "old" else "1"}):
                    ts[arm].append(timeit(fn, 31))
                    if arm not in outs:
                        outs[arm] = fn()
        med = {a: sorted(t)[len(t) // 2] for a, t in ts.items()}
        spread = max(ts["old"]) - min(ts["old"])
        print(json.dumps({"what": "pair_pipe_ab", "kernel": name, "shape": [N, C, H, W], "knob": k["knob"],
                          "old_ms": [round(t, 4) for t in ts["old"]], "new_ms": [round(t, 4) for t in ts["new"]],
                          "old_median_ms": round(med["old"], 4), "new_median_ms": round(med["new"], 4),
                          "old_spread_ms": round(spread, 4), "gain_ms": round(med["old"] - med["new"], 4),
                          "new_wins": bool(med["old"] - med["new"] > spread),
                          "bitwise_equal": bool(torch.equal(outs["old"], outs["new"]))}), flush=True)


if __name__ == "__main__":
    main()
