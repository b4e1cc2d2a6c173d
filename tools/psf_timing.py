#!/usr/bin/env python3
"""
Time and peak memory of the PSF step, fused (metrics.compute_psf(fused=True): tl_psf_accumulate / tl_psf_accumulate_bwd)
against unfused (the default path: two exp tensors [g, w, bins, r] and a batched GEMM, plain torch ops), forward + backward
of sum(kernels * T), on a synthetic fan of F x W x P rays (default 3 x 3 x 2^20 = 9.4 M, 21 x 21 bins).

    python tools/psf_timing.py [--log2-pupil 20] [--bins 21 21] [--runs 7] [--warmup 2] [--out profiles/psf_fused_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included);
the median over the timed runs is reported, with the fused C-ABI calls timed on their own (forward, backward) and
torch.cuda.max_memory_allocated growth of one step of each path.  Development tool, not part of the product.
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
    ap.add_argument("--log2-pupil", type=int, default=20)
    ap.add_argument("--fields", type=int, default=3)
    ap.add_argument("--wavelengths", type=int, default=3)
    ap.add_argument("--bins", type=int, nargs=2, default=(21, 21))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs must be at least 5")
    import torch
    from torchoptics_amd import _lib, metrics, ops
    dev = torch.device("cuda:0")
    F, W, P = a.fields, a.wavelengths, 1 << a.log2_pupil
    nx, ny = a.bins
    n_rays = F * W * P
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.randn((1, F, W, P), generator=g, device=dev) * 0.01).requires_grad_(True)
    y = (torch.randn((1, F, W, P), generator=g, device=dev) * 0.02
         + torch.linspace(0, 3, F, device=dev)[None, :, None, None]).requires_grad_(True)
    ok = (torch.arange(P, device=dev) % 7 != 0).expand(1, F, W, P).contiguous()
    yt = torch.linspace(0, 3, F, device=dev)
    T = torch.randn((F, W, ny, nx), generator=g, device=dev)

    def step(fused):
        x.grad = y.grad = None
        k = metrics.compute_psf(x, y, n_bins=(nx, ny), increment=0.004, y_target=yt, weights=ok, fused=fused)[3]
        (k * T).sum().backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {True: [], False: []}
    for rep in range(a.warmup + a.runs):
        for fused in (True, False):
            t = timed(lambda: step(fused))
            if rep >= a.warmup:
                ms[fused].append(t)
    mem = {}
    for fused in (True, False):
        x.grad = y.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fused)
        torch.cuda.synchronize()
        mem[fused] = torch.cuda.max_memory_allocated() - base

    # the two C-ABI calls on their own
    lib = _lib.lib()
    nxh, x_first = (nx // 2 + 1, 0.0) if nx % 2 else (nx // 2, 0.5)
    xd, yd = x.detach().reshape(F, W, P), y.detach().reshape(F, W, P)
    okb = ok.view(torch.uint8)
    pitch = torch.full((F,), 0.004, device=dev)
    ws = torch.empty(lib.tl_psf_workspace_bytes(F, W, P, nxh, ny), dtype=torch.uint8, device=dev)
    hist = torch.empty((F, W, ny, nxh), device=dev)
    gh = T[..., nx - nxh:].contiguous()
    gx, gy, gp = torch.empty_like(xd), torch.empty_like(yd), torch.empty((3, F), device=dev)
    p = _lib.ptr
    head = (0, F, W, P, p(xd), p(yd), None, p(okb), W * P, P, p(pitch), p(pitch), p(yt), nxh, ny, x_first, 0.5 - ny / 2)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fwd():
        _lib.check(lib.tl_psf_accumulate(*head, p(hist), p(ws), ws.numel(), st), "tl_psf_accumulate")

    def bwd():
        _lib.check(lib.tl_psf_accumulate_bwd(*head, p(gh), p(gx), p(gy), p(gp[0]), p(gp[1]), p(gp[2]), p(ws), ws.numel(), st),
                   "tl_psf_accumulate_bwd")
    calls = {}
    for name, fn in (("tl_psf_accumulate", fwd), ("tl_psf_accumulate_bwd", bwd)):
        for _ in range(a.warmup):
            fn()
        calls[name] = statistics.median(timed(fn) for _ in range(a.runs))

    tf, tu = statistics.median(ms[True]), statistics.median(ms[False])
    fwd_bytes = 9 * n_rays + ws.numel()                     # x, y, ok read once; the partials
    lines = [
        f"PSF step, forward + backward of sum(kernels * T): {F} fields x {W} wavelengths x 2^{a.log2_pupil} rays = {n_rays} rays,"
        f" {nx} x {ny} bins ({ny} x {nxh} half kernel), {torch.cuda.get_device_name(dev)}",
        f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and unfused alternating in one process",
        f"  fused    {tf:9.3f} ms   (min {min(ms[True]):.3f})",
        f"  unfused  {tu:9.3f} ms   (min {min(ms[False]):.3f})",
        f"  ratio unfused / fused  {tu / tf:.2f}",
        "the fused C-ABI calls alone (kernels + launch):",
        f"  tl_psf_accumulate      {calls['tl_psf_accumulate']:9.3f} ms   {calls['tl_psf_accumulate'] * 1e6 / n_rays:.3f} ns per ray,"
        f" {fwd_bytes / calls['tl_psf_accumulate'] / 1e6:.1f} GB/s of the 9 B per ray it reads",
        f"  tl_psf_accumulate_bwd  {calls['tl_psf_accumulate_bwd']:9.3f} ms   {calls['tl_psf_accumulate_bwd'] * 1e6 / n_rays:.3f} ns per ray,"
        f" {17 * n_rays / calls['tl_psf_accumulate_bwd'] / 1e6:.1f} GB/s of the 17 B per ray it moves",
        "peak growth of torch.cuda.max_memory_allocated over one step:",
        f"  fused    {mem[True] / n_rays:7.1f} B per ray   ({mem[True] / 2**20:.0f} MiB)",
        f"  unfused  {mem[False] / n_rays:7.1f} B per ray   ({mem[False] / 2**20:.0f} MiB)",
        f"workspace of the fused calls: {ws.numel()} B = {ws.numel() / n_rays:.4f} B per ray",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
