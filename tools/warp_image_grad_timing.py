#!/usr/bin/env python3
"""
Time and peak memory of imaging.warp_bicubic with the gradient to the IMAGE: fused (tl_warp_fwd, tl_warp_bwd and the
fixed-point scatter tl_warp_bwd_image, image_grad="fused") against the torch formulation (fused=False: 16 advanced-index
gathers forward, 16 float-atomic index_put_ passes backward), forward + backward of sum(out * T) to image, x, y and gain, on
the recorded warp workload: B x 512 x 512 x 3 -> 512 x 512 through the barrel map of a +-5 % distortion profile with a radial
gain, at B = 1 and B = 8.

    python tools/warp_image_grad_timing.py [--runs 7] [--warmup 2] [--out profiles/warp_image_grad_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included); the
median over the timed runs is reported, with the growth of torch.cuda.max_memory_allocated over one step of each path.  Then
tl_warp_bwd_image alone, "auto" (LDS box) and "direct" (global atomics only), each timed window holding --calls calls, against
the time of reading g_out, x, y and gain once and writing g_image once at the measured HBM copy rate.  Development tool, not
part of the product.
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
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="C-ABI calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs must be at least 5")
    import torch
    from torchoptics_amd import _lib, imaging, ops
    dev = torch.device("cuda:0")
    (H, W), Cc = a.size, 3
    fields = (0.25, 0.5, 0.75, 1.0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"warp_bicubic, forward + backward of sum(out * T) to image, x, y and gain: B x {H} x {W} x {Cc} image -> {H} x {W}, barrel "
             f"map (+-5 % distortion, coordinates [1,Ho,Wo]) and a radial gain [1,Ho,Wo,{Cc}], {torch.cuda.get_device_name(dev)}",
             f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused (image_grad='fused') and torch (fused=False) "
             "alternating in one process"]
    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        image = torch.rand((B, H, W, Cc), generator=g, device=dev).requires_grad_(True)
        T = torch.rand((B, H, W, Cc), generator=g, device=dev)
        d = torch.tensor([[0.05, -0.01, -0.03, -0.05]], device=dev)
        ri = torch.tensor([[[0.98, 0.97, 0.99], [0.9, 0.88, 0.92], [0.8, 0.75, 0.82], [0.6, 0.55, 0.65]]], device=dev)
        x, y = (v.detach().requires_grad_(True) for v in imaging.distortion_grid(d, fields, (H, W)))
        gain = imaging.radial_map(ri, fields, (H, W), 1.0).detach().requires_grad_(True)
        leaves = (image, x, y, gain)

        def step(fused):
            for v in leaves:
                v.grad = None
            (imaging.warp_bicubic(image, x, y, gain, fused=fused, image_grad="fused") * T).sum().backward()

        ms = {True: [], False: []}
        for rep in range(a.warmup + a.runs):
            for fused in (True, False):
                t = timed(lambda: step(fused))
                if rep >= a.warmup:
                    ms[fused].append(t)
        mem, grads = {}, {}
        for fused in (True, False):
            for v in leaves:
                v.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(fused)
            torch.cuda.synchronize()
            mem[fused] = torch.cuda.max_memory_allocated() - base
            grads[fused] = [v.grad.clone() for v in leaves]
        agree = max(float((p - q).norm() / q.norm()) for p, q in zip(grads[True], grads[False]))
        tf, tu = statistics.median(ms[True]), statistics.median(ms[False])
        lines += [f"B = {B}",
                  f"  fused  {tf:9.3f} ms   (min {min(ms[True]):.3f})   peak memory growth {mem[True] / 2**20:8.1f} MiB (the workspace, "
                  "8 bytes per image element and grown once, is held by the library's cache and not counted after the first step)",
                  f"  torch  {tu:9.3f} ms   (min {min(ms[False]):.3f})   peak memory growth {mem[False] / 2**20:8.1f} MiB",
                  f"  ratio torch / fused  {tu / tf:.2f}      (gradients of the two paths agree to rel-L2 {agree:.1e})",
                  f"  CONDITION fused median below torch median: {'met' if tf < tu else 'NOT MET'}"]
        # the new C-ABI call on its own, with and without the LDS box
        lib = _lib.lib()
        xd, yd, gd = x.detach(), y.detach(), gain.detach()
        g_image = torch.empty_like(image)
        q = ops.WarpFunction._geom(image, xd, yd, gd)
        nbytes = lib.tl_warp_bwd_image_work_bytes(C.byref(q))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p = _lib.ptr
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        px = H * W
        moved = 4 * (2 * B * px * Cc + 2 * px + px * Cc)                 # g_out, g_image | x, y | gain
        least = moved / HBM * 1e3
        lines.append(f"B = {B}, tl_warp_bwd_image alone (clear + three kernels + launches, workspace {nbytes / 2**20:.1f} MiB), "
                     f"{a.calls} calls per timed window:")
        per_call, results = {}, {}
        for name, flags in (("auto", 0), ("direct", 1)):
            def window():
                for _ in range(a.calls):
                    _lib.check(lib.tl_warp_bwd_image(C.byref(q), p(xd), p(yd), p(gd), p(T), p(g_image), p(work), nbytes, flags, st),
                               "tl_warp_bwd_image")
            for _ in range(a.warmup):
                window()
            per_call[name] = t = statistics.median(timed(window) for _ in range(a.runs)) / a.calls
            results[name] = g_image.clone()
            lines.append(f"  {name:7s} {t * 1e3:9.1f} us per call   {moved / 2**20:7.1f} MiB read once and written once = {least * 1e3:6.1f} us "
                         f"at {HBM / 1e12:.2f} TB/s (measured HBM copy rate): {least / t * 100:5.1f} % of that rate")
        same = bool((results["auto"].view(torch.int32) == results["direct"].view(torch.int32)).all())
        lines.append(f"  auto and direct give the same bits: {same}")
        lines.append(f"  CONDITION auto not slower than direct: {'met' if per_call['auto'] <= per_call['direct'] else 'NOT MET'} "
                     f"(direct / auto = {per_call['direct'] / per_call['auto']:.2f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
