#!/usr/bin/env python3
"""
Time and peak memory of imaging.svola_convolution, fused (the tl_svola_* kernels) against the torch formulation of the same
function (haloed patch stack, one grouped conv2d, weighted accumulate; autograd backward), forward + backward of
sum(out * T), on a synthetic image: 1 x 512 x 512 x 3, grid 5 x 5, PSF 21 x 21, overlap 16, hann -- with the gradient to the
PSFs only, again with the image gradient as well, and both again at B = 8.

    python tools/svola_timing.py [--runs 7] [--warmup 2] [--out profiles/svola_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included); the
median over the timed runs is reported, with the three fused C-ABI calls timed on their own and the growth of
torch.cuda.max_memory_allocated over one step of each path.  Development tool, not part of the product.
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
    ap.add_argument("--grid", type=int, nargs=2, default=(5, 5))
    ap.add_argument("--taps", type=int, nargs=2, default=(21, 21))
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--window", default="hann")
    ap.add_argument("--batches", type=int, nargs="+", default=(1, 8))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs must be at least 5")
    import torch
    from torchoptics_amd import _lib, imaging, ops
    dev = torch.device("cuda:0")
    (H, W), (gh, gw), (kh, kw), o, Cc = a.size, a.grid, a.taps, a.overlap, 3
    geo = imaging.svola_geometry(H, W, gh, gw, o, o, a.window)
    cover = ((geo.tab_r > 0).sum(0)[o:o + H, None] * (geo.tab_c > 0).sum(0)[None, o:o + W]).mean()
    fma = H * W * Cc * kh * kw * float(cover)
    peak = 157.3e12 / 2                                             # fp32 vector FMAs per second (datasheet)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"svola_convolution, forward + backward of sum(out * T): {H} x {W} x {Cc} image, grid {gh} x {gw}, PSF {kh} x {kw}, "
             f"overlap {o}, {a.window}, {torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and torch alternating in one process",
             f"mean cover {cover:.3f} patches per pixel: {fma / 1e6:.1f} M FMAs per lens each way = {fma / peak * 1e3:.4f} ms at the "
             "fp32 vector peak (157.3 TFLOPS, datasheet)"]
    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        image = torch.rand((B, H, W, Cc), generator=g, device=dev)
        psfs = torch.rand((B, gh * gw, kh, kw, Cc), generator=g, device=dev)
        psfs = (psfs / psfs.sum(dim=(2, 3), keepdim=True)).requires_grad_(True)
        T = torch.rand((B, H, W, Cc), generator=g, device=dev)
        for image_grad in (False, True):
            image.requires_grad_(image_grad)

            def step(fused):
                image.grad = psfs.grad = None
                (imaging.svola_convolution(image, o, psfs, (gh, gw), a.window, fused=fused) * T).sum().backward()

            ms = {True: [], False: []}
            for rep in range(a.warmup + a.runs):
                for fused in (True, False):
                    t = timed(lambda: step(fused))
                    if rep >= a.warmup:
                        ms[fused].append(t)
            mem = {}
            for fused in (True, False):
                image.grad = psfs.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step(fused)
                torch.cuda.synchronize()
                mem[fused] = torch.cuda.max_memory_allocated() - base
            tf, tu = statistics.median(ms[True]), statistics.median(ms[False])
            lines += [f"B = {B}, gradient to the PSFs" + (" and the image" if image_grad else " only"),
                      f"  fused  {tf:9.3f} ms   (min {min(ms[True]):.3f})   peak memory growth {mem[True] / 2**20:8.1f} MiB",
                      f"  torch  {tu:9.3f} ms   (min {min(ms[False]):.3f})   peak memory growth {mem[False] / 2**20:8.1f} MiB",
                      f"  ratio torch / fused  {tu / tf:.2f}"]
        # the three C-ABI calls on their own
        image.requires_grad_(False)
        lib = _lib.lib()
        pd = psfs.detach()
        q = ops.SvolaFunction._geom(geo, image, pd, pd)
        wr, wc = ops.SvolaFunction._tables(geo, dev)
        nbytes = lib.tl_svola_workspace_bytes(C.byref(q), *geo.bounds)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out, g_psfs, g_image = torch.empty_like(image), torch.empty_like(pd), torch.empty_like(image)
        p = _lib.ptr
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        head = (C.byref(q), *geo.bounds, p(wr), p(wc))
        calls = {
            "tl_svola_fwd": lambda: lib.tl_svola_fwd(*head, p(image), p(pd), p(out), st),
            "tl_svola_bwd_psf": lambda: lib.tl_svola_bwd_psf(*head, p(image), p(T), p(g_psfs), p(ws), ws.numel(), st),
            "tl_svola_bwd_image": lambda: lib.tl_svola_bwd_image(*head, p(pd), p(T), p(g_image), p(ws), ws.numel(), st),
        }
        lines.append(f"B = {B}, the fused C-ABI calls alone (kernels + launch); workspace {nbytes / 2**20:.1f} MiB:")
        for name, fn in calls.items():
            for _ in range(a.warmup):
                _lib.check(fn(), name)
            t = statistics.median(timed(fn) for _ in range(a.runs))
            lines.append(f"  {name:20s} {t:9.3f} ms   {B * fma / t / 1e9:8.2f} T FMA/s = {B * fma / t * 1e3 / peak * 100:5.1f} % of the "
                         "vector peak")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
