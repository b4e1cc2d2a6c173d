#!/usr/bin/env python3
"""
Time and peak memory of metrics.geometric_mtf, fused (the tl_mtf_* kernels) against fused=False (the same definition in
float64 torch ops, which holds the ray x frequency tensors several times over), forward + backward of mtf.sum() to x, y on a
synthetic fan in the tracer's memory layout: 3 fields x 3 wavelengths x 2^20 rays, 16 frequencies x (tangential, sagittal) = 32
vectors (two launches of 16), pooled over the wavelengths about the field's centroid.

    python tools/mtf_timing.py [--log2-rays 20] [--runs 7] [--warmup 2] [--out profiles/mtf_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included); the
median over the timed runs is reported, with the growth of torch.cuda.max_memory_allocated over one step of each path per ray,
and the C-ABI calls alone (ops.enable_timing) against a device-to-device copy rate measured in the same process on the bytes
they must move (9 B per ray read by each; the seed call writes 8 more).
Development tool, not part of the product.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FREQUENCIES = tuple(5.0 * k for k in range(16))


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
    x = (0.02 + 0.008 * w) * r * th.cos() + 2e-3 * (rnd() - 0.5)
    y = 9.0 * f + 0.003 * w * f + (0.02 + 0.008 * w + 0.02 * f) * r * th.sin() + 2e-3 * (rnd() - 0.5)
    ok = (rnd() > 0.05).permute(0, 1, 3, 2)
    leaves = [t.permute(0, 1, 3, 2).detach().requires_grad_(True) for t in (x, y)]                    # [1,F,P,W] views
    del r, th, x, y

    def step(fused):
        for t in leaves:
            t.grad = None
        out = metrics.geometric_mtf(*leaves, ok, FREQUENCIES, fused=fused)
        out.mtf.sum().backward()
        return out.mtf.detach()

    lines = [f"geometric_mtf, {len(FREQUENCIES)} frequencies x (tangential, sagittal) = {2 * len(FREQUENCIES)} vectors, pooled over the wavelengths "
             f"about the field's centroid, forward + backward of mtf.sum() to x, y: {F} fields x {W} wavelengths x 2^{a.log2_rays} rays = "
             f"{n_rays} rays in the tracer's layout, {torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and fused=False alternating in one process"]
    ms = {True: [], False: []}
    for rep in range(a.warmup + a.runs):
        for fused in (True, False):
            t = timed(lambda: step(fused))
            if rep >= a.warmup:
                ms[fused].append(t)
    mem, grads, curve = {}, {}, {}
    for fused in (True, False):
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        curve[fused] = step(fused)
        torch.cuda.synchronize()
        mem[fused] = torch.cuda.max_memory_allocated() - base
        grads[fused] = [t.grad.clone() for t in leaves]
    agree = max(float((p.double() - q.double()).norm() / q.double().norm()) for p, q in zip(grads[True], grads[False]))
    apart = float((curve[True].double() - curve[False].double()).abs().max())
    del grads
    tf, tu = statistics.median(ms[True]), statistics.median(ms[False])
    lines += [f"  fused        {tf:9.3f} ms   (min {min(ms[True]):.3f})   peak memory growth {mem[True] / n_rays:7.1f} B per ray",
              f"  fused=False  {tu:9.3f} ms   (min {min(ms[False]):.3f})   peak memory growth {mem[False] / n_rays:7.1f} B per ray",
              f"  ratio fused=False / fused  {tu / tf:.2f}      (the curves agree to {apart:.1e}, the gradients of the two paths to rel-L2 {agree:.1e})",
              "  tangential MTF of the last field at 0, 25, 50, 75 cycles / mm: " + ", ".join(f"{curve[True][0, -1, 0, k].item():.3f}" for k in (0, 5, 10, 15))]
    # a device-to-device copy of as many bytes as one call reads, in this process
    src = torch.empty(n_rays * 9, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(a.warmup):
        dst.copy_(src)
    t_copy = statistics.median(timed(lambda: dst.copy_(src)) for _ in range(a.runs))
    rate = 2 * src.numel() / (t_copy * 1e-3)
    del src, dst
    lines.append(f"device-to-device copy of {n_rays * 9 / 2**20:.0f} MiB: {t_copy:.3f} ms = {rate / 1e12:.2f} TB/s (read + written)")
    ops.enable_timing(True)
    for _ in range(a.runs):
        step(True)
    call_ms = ops.named_timing_ms()
    ops.enable_timing(False)
    lines.append(f"the fused C-ABI calls alone (mean over {a.runs} steps, events around each call; tl_mtf_sums and tl_mtf_seed run twice per "
                 "step, 16 vectors each; tl_enclosed_centroid gives n and the origin):")
    for name, per_ray in (("tl_enclosed_centroid", 9), ("tl_mtf_sums", 9), ("tl_mtf_seed", 17)):
        least = n_rays * per_ray / rate * 1e3
        lines.append(f"  {name:21s} {call_ms[name] * 1e3:9.1f} us   {per_ray} B per ray = {least * 1e3:7.1f} us at the copy rate: "
                     f"{least / call_ms[name] * 100:5.1f} % of that rate")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
