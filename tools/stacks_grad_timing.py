#!/usr/bin/env python3
"""
Cost of the gradient through the per-surface penalty stacks (ABI 14) against the fused penalty seed, interleaved rounds.

    python tools/stacks_grad_timing.py [--workloads cfg3 cfg3a] [--mode strict] [--rounds 7] [--log2-pupil 24]

Per workload, two losses of the same aggregate=True trace, alternating round by round:
  fused   rms + 0.2 penalty_sum(PenaltyStacks)       -- moment 8: one seed for every ray and row (kPenUniform kernels)
  stacks  rms + 0.2 penalty_sum(dict(stacks))        -- the caller's sum over the lists: a seed per ray, row and term
                                                        (kPenRay kernels), 12 S bytes per ray read back
Reported (median ms over the rounds, device events on the current stream):
  bwd_cabi  the backward C-ABI call alone (walk-back, selective checkpoint pass, reduction) -- ops.timing_ms
  step      forward + loss + backward of the whole caller step
  target    12 S bytes per ray at 4 TB/s: what reading the seeds costs at the HBM rate
Development tool, not part of the product.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["cfg3", "cfg3a"])
    ap.add_argument("--mode", default="strict")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2-pupil", type=int, default=24)
    a = ap.parse_args()
    import bench
    import torchoptics_amd as ta
    from torchoptics_amd import ops, ray_tracing as rt
    res = []
    for wname in a.workloads:
        args, meta, _ = bench.workload(wname, "cuda:0", 1, 0, a.log2_pupil)
        S = meta["S"]
        n_rays = meta["F"] * meta["W"] * meta["P_local"]
        leaves = [args[k] for k in bench.LEAF_NAMES if k in args]
        extra = {k: args[k] for k in ("kappa", "poly") if k in args}

        def step(kind):
            for v in leaves:
                v.grad = None
            out = ta.trace_skew(args["x"], args["y"], args["z"], args["cx"], args["cy"], args["c"], args["t"], args["mu"],
                                args["mask"], True, True, mode=a.mode, **extra)
            rms = ta.compute_rms2d(out[0], out[1], out[4])
            pen = rt.penalty_sum(out[6] if kind == "fused" else dict(out[6]), S)
            (rms + 0.2 * pen).backward()

        times = {k: {"bwd_cabi": [], "step": []} for k in ("fused", "stacks")}
        for r in range(a.warmup + a.rounds):
            for kind in (("fused", "stacks") if r % 2 == 0 else ("stacks", "fused")):
                ops.enable_timing(True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(kind)
                e1.record()
                torch.cuda.synchronize()
                tm = ops.timing_ms()
                ops.enable_timing(False)
                if r >= a.warmup:
                    times[kind]["bwd_cabi"].append(tm["bwd"])
                    times[kind]["step"].append(e0.elapsed_time(e1))
        med = {k: {m: statistics.median(v) for m, v in d.items()} for k, d in times.items()}
        row = dict(workload=wname, mode=a.mode, S=S, rays=n_rays, rounds=a.rounds, median_ms=med,
                   min_ms={k: {m: min(v) for m, v in d.items()} for k, d in times.items()},
                   bwd_extra_ms=med["stacks"]["bwd_cabi"] - med["fused"]["bwd_cabi"],
                   step_extra_ms=med["stacks"]["step"] - med["fused"]["step"],
                   target_ms=12.0 * S * n_rays / 4e12 * 1e3)
        print(json.dumps(row), flush=True)
        res.append(row)
        del args, leaves
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
