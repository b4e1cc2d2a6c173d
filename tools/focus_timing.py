#!/usr/bin/env python3
"""
Time and peak memory of metrics.through_focus, fused (the tl_focus_* kernels) against fused=False (the same definition in
float64 torch ops), forward + backward of rms_best.sum() to x, y, cx, cy on a synthetic fan in the tracer's memory layout:
3 fields x 3 wavelengths x 2^20 rays.

    python tools/focus_timing.py [--log2-rays 20] [--runs 7] [--warmup 2] [--out profiles/focus_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included); the
median over the timed runs is reported, with the growth of torch.cuda.max_memory_allocated over one step of each path per ray,
the two C-ABI calls alone (ops.enable_timing) against a device-to-device copy rate measured in the same process on the bytes
they must move (17 B per ray forward; 17 read + 16 written backward), and the host time of the float64 finish on the moments
of 256 lenses x 8 fields x 3 wavelengths (forward + backward): the evidence for or against a finish kernel.
Development tool, not part of the product.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    px, py = r * th.cos(), r * th.sin()
    f = torch.linspace(0, 1, F, device=dev).reshape(1, F, 1, 1)
    w = torch.arange(W, device=dev, dtype=torch.float32).reshape(1, 1, W, 1)
    u, v = 0.17 * px, 0.17 * py + 0.35 * f
    x = -(0.12 + 0.05 * w - 0.08 * f) * u + 2e-3 * (rnd() - 0.5)
    y = 9.0 * f - (0.12 + 0.05 * w + 0.11 * f) * (v - 0.35 * f) + 2e-3 * (rnd() - 0.5)
    cz = torch.rsqrt(1 + u * u + v * v)
    ok = (rnd() > 0.05).permute(0, 1, 3, 2)
    leaves = [t.permute(0, 1, 3, 2).detach().requires_grad_(True) for t in (x, y, u * cz, v * cz)]    # [1,F,P,W] views
    del r, th, px, py, u, v, x, y, cz

    def step(fused):
        for t in leaves:
            t.grad = None
        metrics.through_focus(*leaves, ok, fused=fused).rms_best.sum().backward()

    ms = {True: [], False: []}
    for rep in range(a.warmup + a.runs):
        for fused in (True, False):
            t = timed(lambda: step(fused))
            if rep >= a.warmup:
                ms[fused].append(t)
    mem, grads = {}, {}
    for fused in (True, False):
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fused)
        torch.cuda.synchronize()
        mem[fused] = torch.cuda.max_memory_allocated() - base
        grads[fused] = [t.grad.clone() for t in leaves]
    agree = max(float((p.double() - q.double()).norm() / q.double().norm()) for p, q in zip(grads[True], grads[False]))
    del grads
    tf, tu = statistics.median(ms[True]), statistics.median(ms[False])
    lines = [f"through_focus, forward + backward of rms_best.sum() to x, y, cx, cy: {F} fields x {W} wavelengths x 2^{a.log2_rays} rays "
             f"= {n_rays} rays in the tracer's layout, {torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and fused=False alternating in one process",
             f"  fused        {tf:9.3f} ms   (min {min(ms[True]):.3f})   peak memory growth {mem[True] / n_rays:7.1f} B per ray",
             f"  fused=False  {tu:9.3f} ms   (min {min(ms[False]):.3f})   peak memory growth {mem[False] / n_rays:7.1f} B per ray",
             f"  ratio fused=False / fused  {tu / tf:.2f}      (gradients of the two paths agree to rel-L2 {agree:.1e})"]
    # a device-to-device copy of as many bytes as the forward reads, in this process
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
        step(True)
    call_ms = ops.named_timing_ms()
    ops.enable_timing(False)
    lines.append(f"the fused C-ABI calls alone (mean of {a.runs} calls, events around each call):")
    for name, per_ray in (("tl_focus_moments", 17), ("tl_focus_seed", 33)):
        least = n_rays * per_ray / rate * 1e3
        lines.append(f"  {name:17s} {call_ms[name] * 1e3:9.1f} us   {per_ray} B per ray = {least * 1e3:7.1f} us at the copy rate: "
                     f"{least / call_ms[name] * 100:5.1f} % of that rate")
    # the float64 finish on the moments of a minibatch: host time, forward + backward
    B, Fb = 256, 8
    M = (torch.rand((B, Fb, W, 11), generator=g, device=dev, dtype=torch.float64) + 1.0)
    M[..., 0] = 1024.0
    M[..., 5:9] += 2048.0                                       # second moments above the squared means: positive variances
    M.requires_grad_(True)

    def finish():
        M.grad = None
        t0 = time.perf_counter()
        metrics.through_focus_from_moments(M, ("wavelength",), "row", torch.float32).rms_best.sum().backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(a.warmup):
        finish()
    t_fin = statistics.median(finish() for _ in range(a.runs))
    lines.append(f"float64 finish in torch ops, {B} lenses x {Fb} fields x {W} wavelengths, forward + backward, host clock to the "
                 f"synchronise: {t_fin:.3f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
