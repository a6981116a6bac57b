"""What the kernel A/B tools (mhsa_bench.py, ffn_bench.py, lnlin_bench.py) share: every arm runs in one process on the
same tensors, warmed up, in alternating runs of `iters` calls timed with device events; per arm the median over the
runs and their min / max are reported, with its normwise difference against an fp64 evaluation of a slice of the
problem, as one JSON line per problem.  GPU only.
"""
import json
import statistics

import torch


def run_us(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def ab(arms, ref_fn, slice_fn, iters, runs):
    """arms: {name: fn}.  ref_fn() is the fp64 reference of the slice slice_fn cuts out of an arm's result.  Returns
    <arm>_vs_fp64_normwise, <arm>_us (median) and <arm>_us_min_max for every arm."""
    res = {}
    with torch.no_grad():
        ref = ref_fn()
        for name, fn in arms.items():
            res[name + "_vs_fp64_normwise"] = float((slice_fn(fn()).cpu().double() - ref).abs().max() / ref.abs().max())
            run_us(fn, iters)  # warm-up
        times = {name: [] for name in arms}
        for _ in range(runs):
            for name, fn in arms.items():
                times[name].append(run_us(fn, iters))
    for name, v in times.items():
        res[name + "_us"] = round(statistics.median(v), 2)
        res[name + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    return res


def emit(res, out):
    """Print one result as a JSON line, and append it to the file `out` if there is one."""
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
