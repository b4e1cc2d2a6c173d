#!/usr/bin/env python3
"""
Time and peak memory of metrics.zernike_fit, fused (the tl_zfit_* kernels) against fused=False (the same definition in float64
torch ops, design-matrix form), forward + backward of (rms_focus + residual).sum() to x, y on a synthetic fan in the tracer's
memory layout with one shared pupil: 3 fields x 3 wavelengths x 2^20 rays, orders 4 and 6.

    python tools/zfit_timing.py [--log2-rays 20] [--runs 5] [--warmup 1] [--out profiles/zfit_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included); the
median over the timed runs is reported, with the growth of torch.cuda.max_memory_allocated over one step of each path per ray,
and the C-ABI calls alone (ops.enable_timing) against a device-to-device copy rate measured in the same process on the bytes
they must move (x, y, ok and the shared pupil's share forward: 9 B per ray; 9 read + 8 written in the seed).
Development tool, not part of the product.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rays", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
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
    r, th = torch.rand((1, 1, P, 1), generator=g, device=dev).sqrt(), 2 * torch.pi * torch.rand((1, 1, P, 1), generator=g, device=dev)
    px, py = r * th.cos(), r * th.sin()                                               # one pupil shared by every row
    f = torch.linspace(0, 1, F, device=dev).reshape(1, F, 1, 1)
    w = torch.arange(W, device=dev, dtype=torch.float32).reshape(1, 1, W, 1)
    pm, qm = px.reshape(1, 1, 1, P), py.reshape(1, 1, 1, P)                           # the tracer's memory: P contiguous
    rho2 = pm * pm + qm * qm
    noise = lambda: 2e-4 * (torch.rand((1, F, W, P), generator=g, device=dev) - 0.5)  # noqa: E731
    x = (0.01 + 0.004 * w) * pm + 0.02 * rho2 * pm + 0.006 * f * pm * qm + noise()    # defocus, spherical, coma
    y = 9.0 * f + (0.01 + 0.004 * w) * qm + 0.02 * rho2 * qm + 0.003 * f * (rho2 + 2 * qm * qm) + noise()
    ok = (torch.rand((1, F, W, P), generator=g, device=dev) > 0.05).permute(0, 1, 3, 2)
    leaves = [t.permute(0, 1, 3, 2).detach().requires_grad_(True) for t in (x, y)]    # [1,F,P,W] views
    del r, th, pm, qm, rho2, x, y
    lines = [f"zernike_fit, forward + backward of (rms_focus + residual).sum() to x, y: {F} fields x {W} wavelengths x 2^{a.log2_rays} "
             f"rays = {n_rays} rays in the tracer's layout, one shared pupil, {torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and fused=False alternating in one process"]
    src = torch.empty(n_rays * 9, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(a.warmup + 1):
        dst.copy_(src)
    t_copy = statistics.median(timed(lambda: dst.copy_(src)) for _ in range(a.runs))
    rate = 2 * src.numel() / (t_copy * 1e-3)
    del src, dst
    lines.append(f"device-to-device copy of {n_rays * 9 / 2**20:.0f} MiB: {t_copy:.3f} ms = {rate / 1e12:.2f} TB/s (read + written)")
    for order in (4, 6):
        def step(fused):
            for t in leaves:
                t.grad = None
            fit = metrics.zernike_fit(*leaves, ok, px, py, max_order=order, scale=1700.0, fused=fused)
            (fit.rms_focus + fit.residual).sum().backward()

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
        lines += [f"order {order}:",
                  f"  fused        {tf:9.3f} ms   (min {min(ms[True]):.3f})   peak memory growth {mem[True] / n_rays:7.1f} B per ray",
                  f"  fused=False  {tu:9.3f} ms   (min {min(ms[False]):.3f})   peak memory growth {mem[False] / n_rays:7.1f} B per ray",
                  f"  ratio fused=False / fused  {tu / tf:.2f}      (gradients of the two paths agree to rel-L2 {agree:.1e})"]
        ops.enable_timing(True)
        for _ in range(a.runs):
            step(True)
        call_ms = ops.named_timing_ms()
        ops.enable_timing(False)
        lines.append(f"  the fused C-ABI calls alone (mean over {a.runs} steps, events around each call):")
        for name, per_ray in (("tl_zfit_moments", 9), ("tl_zfit_solve", 0), ("tl_zfit_seed", 17)):
            if per_ray:
                least = n_rays * per_ray / rate * 1e3
                lines.append(f"    {name:16s} {call_ms[name] * 1e3:9.1f} us   {per_ray} B per ray = {least * 1e3:7.1f} us at the copy rate: "
                             f"{least / call_ms[name] * 100:5.1f} % of that rate")
            else:
                lines.append(f"    {name:16s} {call_ms[name] * 1e3:9.1f} us   (fit and adjoint calls together; {F * W} rows)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
