"""A/B of the stage-3 conv pair (64 -> 64 -> 64 @56, bs 256, po2 4-bit), JSON lines on stdout.

  python tools/pair64_ab.py kernel
      one conv_pair64 launch (qconv2d_pair) against two single-conv launches (qconv2d twice, each with
      its own weight pack) and the 17-layer stage-3 run through qconv2d_chain against the same run
      with PO2Q_PAIR64=0 left to 17 qconv2d calls; interleaved rounds, HIP events, medians; arms of the
      pair kernel itself: PAIR_AB_ARMS="PO2Q_PAIR64_NTS=3;PO2Q_PAIR64_NTS=0" (';' between arms)
  python tools/pair64_ab.py bench --parent DIR [--rounds 5] [-- bench.py arguments]
      the headline: `python bench.py --gpus 1` in DIR (a built checkout of the parent commit) and in
      this tree, alternated, one JSON line per run and a summary (every round of the new arm against
      every round of the parent arm; the mean gain over the parent arm's spread); with --dump-outputs
      in both arms, the logits compared against the parity tolerance (normwise 1e-5)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def env_arm(arm):
    return dict(kv.split("=", 1) for kv in arm.split(",") if kv)


class scoped_env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def kernel(args):
    import torch

    from po2_quantization_amd import _lib
    from tools.tile_sweep import timeit

    N, H, C, L = args.batch, args.image, 64, 17
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(N, C, H, H, generator=g)).to(dev)
    ws = [(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5).to(dev) for _ in range(L)]
    conv = lambda a, w: _lib.qconv2d(a, w, None, 1, 1, 1, 1, 4, "po2")  # noqa: E731

    def singles(n):
        a = x
        for w in ws[:n]:
            a = conv(a, w)
        return a

    arms = [a for a in os.environ.get("PAIR_AB_ARMS", "PO2Q_PAIR64_NTS=3").split(";") if a]
    fns = {"two_singles": (lambda: singles(2), {}), "singles17": (lambda: singles(L), {})}
    for arm in arms:
        fns["pair[%s]" % arm] = (lambda: _lib.qconv2d_pair(x, ws[0], ws[1], 4, "po2"), env_arm(arm))
        fns["chain17[%s]" % arm] = (lambda: _lib.qconv2d_chain(x, ws, 4, "po2"), env_arm(arm))
    res, outs = {}, {}
    for _ in range(args.rounds):
        for name, (fn, env) in fns.items():
            with scoped_env(env):
                res.setdefault(name, []).append(timeit(fn, 11))
                if name not in outs:
                    outs[name] = fn()
    flops2 = 2 * 2.0 * N * C * H * H * C * 9
    for name, ts in res.items():
        ms = sorted(ts)[len(ts) // 2]
        layers = 2 if name.startswith(("pair", "two")) else L
        ref = outs["two_singles" if layers == 2 else "singles17"]
        print(json.dumps({"what": "kernel", "arm": name, "batch": N, "H": H, "layers": layers, "ms": round(ms, 4),
                          "all_ms": [round(t, 4) for t in ts],
                          "eff_mfma_frac": round(flops2 * layers / 2 / (ms * 1e-3) / (2516.6e12 / 3), 3),
                          "bitwise_equal_singles": bool(torch.equal(outs[name], ref))}), flush=True)


def bench(args):
    import numpy as np

    trees = {"parent": os.path.abspath(args.parent), "new": ROOT}
    vals = {k: [] for k in trees}
    for r in range(args.rounds):
        for arm in (("parent", "new") if r % 2 == 0 else ("new", "parent")):
            cmd = [sys.executable, "bench.py", "--gpus", "1"] + args.bench_args
            if args.dump and r == args.rounds - 1:
                cmd += ["--dump-outputs", os.path.join(os.path.abspath(args.dump), arm)]
            out = subprocess.run(cmd, cwd=trees[arm], check=True, capture_output=True, text=True,
                                 timeout=args.run_timeout).stdout
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            vals[arm].append(rec["value"])
            print(json.dumps({"what": "bench", "arm": arm, "round": r, "images_per_s": rec["value"],
                              "ms_per_step": rec.get("ms_per_step")}), flush=True)
    p, n = vals["parent"], vals["new"]
    spread = max(p) - min(p)
    gain = sum(n) / len(n) - sum(p) / len(p)
    summary = {"what": "bench_summary", "parent": p, "new": n, "parent_mean": round(sum(p) / len(p), 1),
               "new_mean": round(sum(n) / len(n), 1), "mean_gain": round(gain, 1),
               "mean_gain_pct": round(100.0 * gain / (sum(p) / len(p)), 2), "parent_spread": round(spread, 1),
               "gain_over_parent_spread": round(gain / spread, 2) if spread > 0 else None,
               "every_new_round_beats_every_parent_round": min(n) > max(p)}
    if args.dump:
        a = np.load(os.path.join(args.dump, "parent", "logits.npy")).astype(np.float64)
        b = np.load(os.path.join(args.dump, "new", "logits.npy")).astype(np.float64)
        summary["logits_normwise_diff"] = float(np.abs(a - b).max() / np.abs(a).max())
        summary["logits_within_1e-5"] = summary["logits_normwise_diff"] <= 1e-5
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "bench"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--image", type=int, default=56)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="bench: a built checkout of the parent commit")
    ap.add_argument("--dump", default=None, help="bench: directory for both arms' --dump-outputs (last round)")
    ap.add_argument("--run-timeout", type=float, default=240.0)
    ap.add_argument("bench_args", nargs="*", help="bench: further bench.py arguments (after --)")
    args = ap.parse_args()
    if args.what == "kernel":
        kernel(args)
    else:
        if not args.parent:
            raise SystemExit("bench needs --parent DIR")
        bench(args)


if __name__ == "__main__":
    main()
