#!/usr/bin/env python3
"""
Time and peak memory of imaging.ms_ssim, fused (the tl_ms_ssim_* calls) against the torch formulation of the same function
(per level ten grouped 1-D conv2d calls, the elementwise maps, the pooling; autograd backward), forward + backward of
sum(ms_ssim) with the gradient to `a` only and to both images, on synthetic images of B x 512 x 512 x 3 at B = 1 and B = 8 (tf's
defaults: five levels, window 11): a smooth field plus 1 % noise against its slightly different twin.

    python tools/ms_ssim_timing.py [--runs 9] [--warmup 3] [--out profiles/ms_ssim_timing.txt]

The protocol is tools/ssim_timing.py's: the two paths alternate in one process; each run is timed with device events around
the whole step (host chain included); the median over the timed runs is reported, with the growth of
torch.cuda.max_memory_allocated over one step of each path, and the C-ABI calls timed on their own (each timed window holds
--calls calls).  The single-scale imaging.ssim figures are taken in the same run for context.  Development tool, not part of the
product.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512))
    ap.add_argument("--batches", type=int, nargs="+", default=(1, 8))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50, help="C-ABI calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs must be at least 5")
    import torch
    from torchoptics_amd import _lib, imaging, ops
    dev = torch.device("cuda:0")
    (H, W), Cc = a.size, 3
    power = imaging.MS_SSIM_POWER_FACTORS
    M = len(power)
    sizes = imaging.ms_ssim_level_sizes(H, W, M)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"ms_ssim, forward + backward of sum(ms_ssim): two B x {H} x {W} x {Cc} float32 images (a smooth field plus 1 % noise "
             f"each), {M} levels ({', '.join(f'{h} x {w}' for h, w in sizes)}), window 11, sigma 1.5, "
             f"{torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and torch alternating in one process; "
             "the ssim lines are the single-scale imaging.ssim in the same run"]
    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                                indexing="ij")
        field = (0.5 + 0.3 * torch.sin(0.05 * xx) * torch.cos(0.04 * yy))[None, :, :, None].expand(B, H, W, Cc)
        img_a = (field + 0.01 * torch.randn((B, H, W, Cc), generator=g, device=dev)).contiguous()
        img_b = (field + 0.01 * torch.randn((B, H, W, Cc), generator=g, device=dev)).contiguous()
        for needs in (("a",), ("a", "b")):
            ta, tb = img_a.clone().requires_grad_("a" in needs), img_b.clone().requires_grad_("b" in needs)
            lines.append(f"B = {B}, gradient to {' and '.join(needs)}")
            for label, merit in (("ms_ssim", imaging.ms_ssim), ("ssim", imaging.ssim)):
                def step(fused):
                    ta.grad = tb.grad = None
                    merit(ta, tb, fused=fused).sum().backward()

                ms = {True: [], False: []}
                for rep in range(a.warmup + a.runs):
                    for fused in (True, False):
                        t = timed(lambda: step(fused))
                        if rep >= a.warmup:
                            ms[fused].append(t)
                mem, grads = {}, {}
                for fused in (True, False):
                    ta.grad = tb.grad = None
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    step(fused)
                    torch.cuda.synchronize()
                    mem[fused] = torch.cuda.max_memory_allocated() - base
                    grads[fused] = [v.grad.clone() for v in (ta, tb) if v.grad is not None]
                agree = max(float((p - q).norm() / q.norm()) for p, q in zip(grads[True], grads[False]))
                tf, tu = statistics.median(ms[True]), statistics.median(ms[False])
                lines += [f"  {label:8s} fused  {tf:9.3f} ms   (min {min(ms[True]):.3f})   peak memory growth {mem[True] / 2**20:8.1f} MiB",
                          f"  {label:8s} torch  {tu:9.3f} ms   (min {min(ms[False]):.3f})   peak memory growth {mem[False] / 2**20:8.1f} MiB",
                          f"  {label:8s} ratio torch / fused  {tu / tf:.2f}   memory fused / torch  {mem[True] / mem[False]:.2f}"
                          f"      (gradients of the two paths agree to rel-L2 {agree:.1e})"]
        # the C-ABI calls on their own
        lib = _lib.lib()
        window = tuple(float(v) for v in imaging.ssim_window(11, 1.5, torch.float32))
        p = _lib.ptr
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        value, g_value, g_p = torch.empty(B, device=dev), torch.ones(B, device=dev), torch.empty_like(img_a)
        terms = torch.empty((B, Cc, M), device=dev)
        q0 = ops.MsSsimFunction._geom(img_a, img_b, window, 1e-4, 9e-4, power, 0)
        q3 = ops.MsSsimFunction._geom(img_a, img_b, window, 1e-4, 9e-4, power, 3, g=g_p)
        keep = torch.empty(lib.tl_ms_ssim_keep_elems(C.byref(q3)), device=dev)
        ws = torch.empty(lib.tl_ms_ssim_work_bytes(C.byref(q3)), dtype=torch.uint8, device=dev)
        s0 = ops.SsimFunction._geom(img_a, img_b, window, 1e-4, 9e-4, flags=0)
        s3 = ops.SsimFunction._geom(img_a, img_b, window, 1e-4, 9e-4, flags=3, g=g_p)
        n = lib.tl_ssim_maps_elems(C.byref(s0))
        maps = [torch.empty(n, device=dev) for _ in range(5)]
        sws = torch.empty(lib.tl_ssim_work_bytes(C.byref(s0)), dtype=torch.uint8, device=dev)
        calls = {
            "tl_ms_ssim_fwd, no maps": (lambda: lib.tl_ms_ssim_fwd(C.byref(q0), p(img_a), p(img_b), p(value), p(terms), p(keep),
                                                                     keep.numel(), p(ws), ws.numel(), st), 2 * M),
            "tl_ms_ssim_fwd, maps of both": (lambda: lib.tl_ms_ssim_fwd(C.byref(q3), p(img_a), p(img_b), p(value), p(terms), p(keep),
                                                                          keep.numel(), p(ws), ws.numel(), st), 2 * M),
            "tl_ms_ssim_bwd": (lambda: lib.tl_ms_ssim_bwd(C.byref(q3), p(img_a), p(img_b), p(keep), keep.numel(), p(g_value), p(g_p), 0,
                                                          p(ws), ws.numel(), st), M),
            "tl_ssim_fwd, no maps": (lambda: lib.tl_ssim_fwd(C.byref(s0), p(img_a), p(img_b), p(value), None, None, None, None, None,
                                                               p(sws), sws.numel(), st), 2),
            "tl_ssim_fwd, 5 maps": (lambda: lib.tl_ssim_fwd(C.byref(s3), p(img_a), p(img_b), p(value), *[p(m) for m in maps], p(sws),
                                                              sws.numel(), st), 2),
            "tl_ssim_bwd": (lambda: lib.tl_ssim_bwd(C.byref(s3), p(img_a), p(img_b), p(maps[0]), p(maps[1]), p(maps[4]), p(g_value),
                                                     p(g_p), st), 1),
        }
        lines.append(f"B = {B}, the fused C-ABI calls alone (kernels + launch), {a.calls} calls per timed window; the keep buffer for "
                     f"both gradients is {keep.numel() * 4 / 2**20:.1f} MiB = {keep.numel() * 4 / (B * H * W * Cc):.1f} bytes per pixel "
                     "and channel:")
        for name, (fn, launches) in calls.items():
            def run_window():
                for _ in range(a.calls):
                    _lib.check(fn(), name)
            for _ in range(a.warmup):
                run_window()
            t = statistics.median(timed(run_window) for _ in range(a.runs)) / a.calls
            lines.append(f"  {name:30s} {t * 1e3:9.1f} us per call   ({launches} launches)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
