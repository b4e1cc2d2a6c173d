#!/usr/bin/env python3
"""
Time and peak memory of imaging.ssim, fused (the tl_ssim_* kernels) against the torch formulation of the same function (ten
grouped 1-D conv2d calls, the elementwise maps, autograd backward), forward + backward of sum(ssim) with the gradient to `a`
only and to both images, on synthetic images of B x 512 x 512 x 3 at B = 1 and B = 8: a smooth field plus 1 % noise against
its slightly different twin.

    python tools/ssim_timing.py [--runs 9] [--warmup 3] [--out profiles/ssim_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included); the
median over the timed runs is reported, with the growth of torch.cuda.max_memory_allocated over one step of each path, and the
fused forward call without partial maps timed on its own (each timed window holds --calls calls) against the time of reading
the two images once at the measured HBM copy rate.  Development tool, not part of the product.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.29e12          # bytes per second: the measured float4 copy rate of the MI355X (8.0 TB/s on the datasheet)


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

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"ssim, forward + backward of sum(ssim): two B x {H} x {W} x {Cc} float32 images (a smooth field plus 1 % noise each), window "
             f"11, sigma 1.5, {torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and torch alternating in one process"]
    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                                indexing="ij")
        field = (0.5 + 0.3 * torch.sin(0.05 * xx) * torch.cos(0.04 * yy))[None, :, :, None].expand(B, H, W, Cc)
        img_a = (field + 0.01 * torch.randn((B, H, W, Cc), generator=g, device=dev)).contiguous()
        img_b = (field + 0.01 * torch.randn((B, H, W, Cc), generator=g, device=dev)).contiguous()
        for needs in (("a",), ("a", "b")):
            ta, tb = img_a.clone().requires_grad_("a" in needs), img_b.clone().requires_grad_("b" in needs)

            def step(fused):
                ta.grad = tb.grad = None
                imaging.ssim(ta, tb, fused=fused).sum().backward()

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
            lines += [f"B = {B}, gradient to {' and '.join(needs)}",
                      f"  fused  {tf:9.3f} ms   (min {min(ms[True]):.3f})   peak memory growth {mem[True] / 2**20:8.1f} MiB",
                      f"  torch  {tu:9.3f} ms   (min {min(ms[False]):.3f})   peak memory growth {mem[False] / 2**20:8.1f} MiB",
                      f"  ratio torch / fused  {tu / tf:.2f}      (gradients of the two paths agree to rel-L2 {agree:.1e})"]
        # the C-ABI calls on their own
        lib = _lib.lib()
        window = tuple(float(v) for v in imaging.ssim_window(11, 1.5, torch.float32))
        p = _lib.ptr
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        value, g_value, g_p = torch.empty(B, device=dev), torch.ones(B, device=dev), torch.empty_like(img_a)
        q0 = ops.SsimFunction._geom(img_a, img_b, window, 1e-4, 9e-4, flags=0)
        q3 = ops.SsimFunction._geom(img_a, img_b, window, 1e-4, 9e-4, flags=3, g=g_p)
        n = lib.tl_ssim_maps_elems(C.byref(q0))
        maps = [torch.empty(n, device=dev) for _ in range(5)]
        ws = torch.empty(lib.tl_ssim_work_bytes(C.byref(q0)), dtype=torch.uint8, device=dev)
        image_bytes, map_bytes = 4 * B * H * W * Cc, 4 * n
        calls = {
            "tl_ssim_fwd, no maps": (lambda: lib.tl_ssim_fwd(C.byref(q0), p(img_a), p(img_b), p(value), None, None, None, None, None,
                                                               p(ws), ws.numel(), st), 2 * image_bytes, "two images read once"),
            "tl_ssim_fwd, 5 maps": (lambda: lib.tl_ssim_fwd(C.byref(q3), p(img_a), p(img_b), p(value), *[p(m) for m in maps], p(ws),
                                                              ws.numel(), st), 2 * image_bytes + 5 * map_bytes,
                                    "two images read, five maps written once"),
            "tl_ssim_bwd": (lambda: lib.tl_ssim_bwd(C.byref(q3), p(img_a), p(img_b), p(maps[0]), p(maps[1]), p(maps[4]), p(g_value),
                                                     p(g_p), st), 3 * image_bytes + 3 * map_bytes,
                            "three maps and two images read, one gradient written once"),
        }
        lines.append(f"B = {B}, the fused C-ABI calls alone (kernels + launch), {a.calls} calls per timed window:")
        for name, (fn, moved, what) in calls.items():
            def run_window():
                for _ in range(a.calls):
                    _lib.check(fn(), name)
            for _ in range(a.warmup):
                run_window()
            t = statistics.median(timed(run_window) for _ in range(a.runs)) / a.calls
            least = moved / HBM * 1e3
            lines.append(f"  {name:22s} {t * 1e3:9.1f} us per call   {moved / 2**20:7.1f} MiB ({what}) = {least * 1e3:6.1f} us "
                         f"at {HBM / 1e12:.2f} TB/s (measured HBM copy rate): {least / t * 100:5.1f} % of that rate")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
