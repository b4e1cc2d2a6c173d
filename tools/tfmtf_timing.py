#!/usr/bin/env python3
"""
Time and peak memory of metrics.through_focus_mtf, forward + backward of mtf.sum() to x, y, cx, cy on a synthetic fan in the
tracer's memory layout: 3 fields x 3 wavelengths x 2^20 rays, frequencies (20, 40) cycles / mm x (tangential, sagittal) = 4
vectors, 16 planes over +-0.15 mm, pooled over the wavelengths about the field's centroid.  Three paths alternate in one process:
  (a) fused          the tl_tfmtf_* kernels: one pass, a rotor per ray and frequency vector;
  (b) plane loop     what a user could do before them: per plane x + d cx / cz, y + d cy / cz in torch (float32, as the rays are)
                     and geometric_mtf(fused=True), the rays read once per plane;
  (c) fused=False    the definition in float64 torch ops.

    python tools/tfmtf_timing.py [--log2-rays 20] [--runs 7] [--warmup 2] [--out profiles/tfmtf_timing.txt]

Each run is timed with device events around the whole step (host chain included); the median over the timed runs is reported,
with the growth of torch.cuda.max_memory_allocated over one step of each path per ray, and the two C-ABI calls alone
(ops.enable_timing) against a device-to-device copy rate measured in the same process on the 17 B per ray they must read (the
seed call writes 16 more).
Development tool, not part of the product.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FREQUENCIES = (20.0, 40.0)
PLANES = (-0.15, 0.02, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rays", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs must be at least 5")
    import torch
    from torchoptics_amd import metrics, ops
    dev = torch.device("cuda:0")
    F, W, P = 3, 3, 1 << a.log2_rays
    n_rays = F * W * P

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda: torch.rand((1, F, W, P), generator=g, device=dev)                 # noqa: E731  (the tracer's memory: P contiguous)
    r, th = rnd().sqrt(), 2 * torch.pi * rnd()
    f = torch.linspace(0, 1, F, device=dev).reshape(1, F, 1, 1)
    w = torch.arange(W, device=dev, dtype=torch.float32).reshape(1, 1, W, 1)
    u, v = 0.17 * r * th.cos(), 0.17 * r * th.sin() + 0.35 * f                      # an f / 3 cone, chief ray at 19 degrees at the edge
    zs, zt = 0.03 + 0.02 * w - 0.04 * f, 0.03 + 0.02 * w + 0.05 * f                 # sagittal / tangential foci inside the planes
    x = -zs * u + 2e-3 * (rnd() - 0.5)
    y = 9.0 * f + 0.003 * w * f - zt * (v - 0.35 * f) + 2e-3 * (rnd() - 0.5)
    cz = 1.0 / torch.sqrt(1 + u * u + v * v)
    ok = (rnd() > 0.05).permute(0, 1, 3, 2)
    leaves = [t.permute(0, 1, 3, 2).detach().requires_grad_(True) for t in (x, y, u * cz, v * cz)]     # [1,F,P,W] views
    del r, th, x, y, u, v, cz

    def plane_loop():
        x, y, cx, cy = leaves
        cz = torch.sqrt(1 - cx * cx - cy * cy)
        u, v = cx / cz, cy / cz
        return torch.stack([metrics.geometric_mtf(x + d * u, y + d * v, ok, FREQUENCIES, fused=True).mtf
                            for d in metrics.plane_shifts(PLANES)], dim=2)

    paths = {"fused": lambda: metrics.through_focus_mtf(*leaves, ok, FREQUENCIES, PLANES, fused=True).mtf, "plane loop": plane_loop,
             "fused=False": lambda: metrics.through_focus_mtf(*leaves, ok, FREQUENCIES, PLANES, fused=False).mtf}

    def step(path):
        for t in leaves:
            t.grad = None
        mtf = paths[path]()
        mtf.sum().backward()
        return mtf.detach()

    lines = [f"through_focus_mtf, frequencies {FREQUENCIES} x (tangential, sagittal) = {2 * len(FREQUENCIES)} vectors, {PLANES[2]} planes from "
             f"{PLANES[0]} in steps of {PLANES[1]}, pooled over the wavelengths about the field's centroid, forward + backward of mtf.sum() "
             f"to x, y, cx, cy: {F} fields x {W} wavelengths x 2^{a.log2_rays} rays = {n_rays} rays in the tracer's layout, "
             f"{torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, the three paths alternating in one process"]
    ms = {p: [] for p in paths}
    for rep in range(a.warmup + a.runs):
        for p in paths:
            t = timed(lambda: step(p))
            if rep >= a.warmup:
                ms[p].append(t)
    mem, grads, curve = {}, {}, {}
    for p in paths:
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        curve[p] = step(p)
        torch.cuda.synchronize()
        mem[p] = torch.cuda.max_memory_allocated() - base
        grads[p] = [t.grad.clone() for t in leaves]
    med = {p: statistics.median(v) for p, v in ms.items()}
    for p in paths:
        lines.append(f"  {p:12s} {med[p]:9.3f} ms   (min {min(ms[p]):.3f})   peak memory growth {mem[p] / n_rays:7.1f} B per ray")
    spread = max(med[p] - min(ms[p]) for p in ("fused", "plane loop"))
    gain = med["plane loop"] - med["fused"]
    lines += [f"  ratio plane loop / fused  {med['plane loop'] / med['fused']:.2f}     ratio fused=False / fused  {med['fused=False'] / med['fused']:.2f}",
              f"  the plane loop takes {gain:+.3f} ms more than fused; the largest spread between a median and its minimum is {spread:.3f} ms: "
              + ("fused is faster by more than the spread" if gain > spread else "fused is NOT faster by more than the spread"),
              "  largest difference of the curves: fused vs fused=False "
              f"{float((curve['fused'].double() - curve['fused=False'].double()).abs().max()):.1e}, plane loop vs fused=False "
              f"{float((curve['plane loop'].double() - curve['fused=False'].double()).abs().max()):.1e}, plane loop vs fused "
              f"{float((curve['plane loop'].double() - curve['fused'].double()).abs().max()):.1e} (the float32 rounding of the shifted coordinates)"]
    for p in ("fused", "plane loop"):
        agree = max(float((q.double() - s.double()).norm() / s.double().norm()) for q, s in zip(grads[p], grads["fused=False"]))
        lines.append(f"  gradients of {p} against fused=False: rel-L2 {agree:.1e}")
    lines.append("  tangential MTF of the last field at 40 cycles / mm over the planes: "
                 + ", ".join(f"{curve['fused'][0, -1, z, 0, 1].item():.3f}" for z in range(PLANES[2])))
    del grads
    # a device-to-device copy of as many bytes as one call reads, in this process
    src = torch.empty(n_rays * 17, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(a.warmup):
        dst.copy_(src)
    t_copy = statistics.median(timed(lambda: dst.copy_(src)) for _ in range(a.runs))
    rate = 2 * src.numel() / (t_copy * 1e-3)
    del src, dst
    lines.append(f"device-to-device copy of {n_rays * 17 / 2**20:.0f} MiB: {t_copy:.3f} ms = {rate / 1e12:.2f} TB/s (read + written)")
    ops.enable_timing(True)
    for _ in range(a.runs):
        step("fused")
    call_ms = ops.named_timing_ms()
    ops.enable_timing(False)
    lines.append(f"the fused C-ABI calls alone (mean over {a.runs} steps, events around each call; tl_tfmtf_sums goes in two launches of 2 "
                 "vectors x 16 planes, each reading the rays; tl_focus_moments gives n and the origin):")
    for name, per_ray, reads in (("tl_focus_moments", 17, 1), ("tl_tfmtf_sums", 17, 2), ("tl_tfmtf_seed", 33, 1)):
        least = n_rays * per_ray * reads / rate * 1e3
        lines.append(f"  {name:21s} {call_ms[name] * 1e3:9.1f} us   {reads} x {per_ray} B per ray = {least * 1e3:7.1f} us at the copy rate: "
                     f"{least / call_ms[name] * 100:5.1f} % of that rate")
    ops.enable_timing(True)
    for _ in range(a.runs):
        step("plane loop")
    loop_ms = ops.named_timing_ms()
    ops.enable_timing(False)
    lines.append(f"the plane loop's C-ABI calls (mean per call; each runs {PLANES[2]} times per step): "
                 + ", ".join(f"{k} {loop_ms[k] * 1e3:.1f} us" for k in ("tl_enclosed_centroid", "tl_mtf_sums", "tl_mtf_seed")))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
