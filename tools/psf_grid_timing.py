#!/usr/bin/env python3
"""
Time and peak memory of the PSF-grid step, fused (imaging.psf_grid_from_trace(fused=True): tl_psf_rot_accumulate /
tl_psf_rot_accumulate_bwd) against fused=False (rotate per term, two exp tensors [term, w, bins, r], a batched GEMM: plain
torch ops), forward + backward of sum(psfs * T), on a synthetic comatic fan of F x W x P rays (default 3 x 3 x 2^18) over a
gh x gw grid (default 5 x 5, linear blend), 21 x 21 bins.

    python tools/psf_grid_timing.py [--log2-pupil 18] [--grid 5 5] [--bins 21 21] [--runs 7] [--warmup 2]
                                    [--out profiles/psf_grid_timing.txt]

The two paths alternate in one process; each run is timed with device events around the whole step (host chain included);
the median over the timed runs is reported, with the two C-ABI calls timed on their own and the growth of
torch.cuda.max_memory_allocated over one step of each path.  If the fused=False step does not fit in memory its fan is halved
until it does, and the size used is stated.  Next to the measurements stand the estimates they are to be read against: the
matrix pipe of the forward (v_mfma_f32_32x32x2_f32 takes two rays in 64 cycles: 32 cycles per ray, term, channel and SIMD) and
the VALU count of the backward.  Development tool, not part of the product.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIMDS, CLOCK_GHZ = 256 * 4, 2.4             # MI355X: 256 CUs of 4 SIMDs, 2.4 GHz peak engine clock


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-pupil", type=int, default=18)
    ap.add_argument("--fields", type=int, default=3)
    ap.add_argument("--wavelengths", type=int, default=3)
    ap.add_argument("--grid", type=int, nargs=2, default=(5, 5))
    ap.add_argument("--bins", type=int, nargs=2, default=(21, 21))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs must be at least 5")
    import torch
    from torchoptics_amd import _lib, imaging
    dev = torch.device("cuda:0")
    F, W = a.fields, a.wavelengths
    nx, ny = a.bins
    gh, gw = a.grid
    fields = tuple(float(v) for v in torch.linspace(0, 1, F))
    cells = imaging.psf_grid_cells((64 * gh, 64 * gw), (gh, gw), 8, fields)
    n_terms = int(cells.src.size)

    def fan(log2_p):
        P = 1 << log2_p
        g = torch.Generator(device=dev).manual_seed(0)
        hf = torch.linspace(0, 1, F, device=dev)[None, :, None, None]
        rho, th = torch.rand((1, F, W, P), generator=g, device=dev).sqrt(), torch.rand((1, F, W, P), generator=g, device=dev) * 6.2831853
        x = 0.01 * rho * torch.cos(th) + 0.01 * hf * rho ** 2 * torch.sin(2 * th)
        y = 3.0 * hf + 0.01 * rho * torch.sin(th) + 0.01 * hf * rho ** 2 * (2 + torch.cos(2 * th))
        ok = (torch.arange(P, device=dev) % 7 != 0).expand(1, F, W, P).contiguous()
        # the tracer's [1, F, P, W] with rays contiguous in memory
        return x.permute(0, 1, 3, 2).requires_grad_(True), y.permute(0, 1, 3, 2).requires_grad_(True), ok.permute(0, 1, 3, 2)

    yt = torch.linspace(0, 3, F, device=dev)
    T = torch.randn((1, cells.N, ny, nx, W), generator=torch.Generator(device=dev).manual_seed(1), device=dev)

    def step(data, fused):
        x, y, ok = data
        x.grad = y.grad = None
        p = imaging.psf_grid_from_trace(x, y, ok, cells, (nx, ny), 0.004, y_target=yt, fused=fused)
        (p * T).sum().backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    data = {True: fan(a.log2_pupil)}
    log2_unfused = a.log2_pupil
    while True:                                             # the largest fan (<= the fused one) whose fused=False step fits
        try:
            data[False] = data[True] if log2_unfused == a.log2_pupil else fan(log2_unfused)
            step(data[False], False)
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            data.pop(False, None)
            torch.cuda.empty_cache()
            log2_unfused -= 1
            if log2_unfused < 8:
                raise
    rays = {True: F * W << a.log2_pupil, False: F * W << log2_unfused}

    ms = {True: [], False: []}
    for rep in range(a.warmup + a.runs):
        for fused in (True, False):
            t = timed(lambda: step(data[fused], fused))
            if rep >= a.warmup:
                ms[fused].append(t)
    mem = {}
    for fused in (True, False):
        data[fused][0].grad = data[fused][1].grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(data[fused], fused)
        torch.cuda.synchronize()
        mem[fused] = torch.cuda.max_memory_allocated() - base

    # the two C-ABI calls on their own
    lib = _lib.lib()
    P = 1 << a.log2_pupil
    x, y, ok = data[True]
    xd, yd = (v.detach().permute(0, 1, 3, 2).reshape(F, W, P) for v in (x, y))
    okb = ok.permute(0, 1, 3, 2).reshape(F, W, P).contiguous().view(torch.uint8)
    assert xd.is_contiguous() and yd.is_contiguous()
    up = lambda v: torch.from_numpy(v).to(dev)              # noqa: E731
    src, c, s, fstart, fgrids = (up(v) for v in (cells.src, cells.c, cells.s, cells.field_start, cells.field_grids))
    pitch = torch.full((n_terms,), 0.004, device=dev)
    nbytes = lib.tl_psf_rot_workspace_bytes(n_terms, F, W, P, nx, ny)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    hist = torch.empty((n_terms, W, ny, nx), device=dev)
    gh_ = torch.randn((n_terms, W, ny, nx), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    gx, gy, gyc = torch.empty_like(xd), torch.empty_like(yd), torch.empty(F, device=dev)
    p = _lib.ptr
    head = (0, n_terms, F, W, P, p(xd), p(yd), None, p(okb), W * P, P, p(src), p(c), p(s), p(pitch), p(pitch), p(yt), nx, ny,
            0.5 - nx / 2, 0.5 - ny / 2)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fwd():
        _lib.check(lib.tl_psf_rot_accumulate(*head, p(hist), p(ws), ws.numel(), st), "tl_psf_rot_accumulate")

    def bwd():
        _lib.check(lib.tl_psf_rot_accumulate_bwd(*head, p(fstart), p(fgrids), p(gh_), p(gx), p(gy), p(gyc), p(ws), ws.numel(), st),
                   "tl_psf_rot_accumulate_bwd")
    calls = {}
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        for _ in range(a.warmup):
            fn()
        calls[name] = statistics.median(timed(fn) for _ in range(a.runs))

    tf, tu = statistics.median(ms[True]), statistics.median(ms[False])
    ray_terms = n_terms * W * P                             # (ray, term, channel) triples: what both kernels' work is counted in
    mfma_ms = ray_terms * 32 / SIMDS / (CLOCK_GHZ * 1e6)
    nxp = (nx + 3) & ~3
    valu = 2 * ny * nxp + 6 * nxp + 6 * ny + 40             # per triple: 2 fma per bin; 2 mul, sub, add, 2 for exp2 per column and row
    trans = nxp + ny                                        # v_exp_f32 per triple, quarter rate
    valu_ms = ray_terms / 64 * (valu * 4 + trans * 16) / SIMDS / (CLOCK_GHZ * 1e6)      # a wave64 VALU op issues in 4 cycles
    per_ray = lambda t, n: t * 1e6 / n                      # noqa: E731
    lines = [
        f"PSF-grid step, forward + backward of sum(psfs * T): {F} fields x {W} wavelengths x 2^{a.log2_pupil} rays = {rays[True]} rays,"
        f" {gh} x {gw} grid, linear blend = {n_terms} terms (rotated grids), {nx} x {ny} bins, {torch.cuda.get_device_name(dev)}",
        f"median of {a.runs} event-timed runs after {a.warmup} warm-up rounds, fused and fused=False alternating in one process",
        f"  fused        {tf:9.3f} ms   (min {min(ms[True]):.3f})   {rays[True]} rays",
        f"  fused=False  {tu:9.3f} ms   (min {min(ms[False]):.3f})   {rays[False]} rays (2^{log2_unfused} per channel"
        + (")" if log2_unfused == a.log2_pupil else f": the fan was halved until the step fit in memory)"),
        f"  ratio fused=False / fused, per ray  {per_ray(tu, rays[False]) / per_ray(tf, rays[True]):.2f}",
        f"the fused C-ABI calls alone (kernels + launch), {ray_terms} (ray, term, channel) triples:",
        f"  tl_psf_rot_accumulate      {calls['fwd']:9.3f} ms   {calls['fwd'] * 1e6 / ray_terms:.4f} ns per triple;"
        f" matrix-pipe estimate (32 MFMA cycles per triple and SIMD, {SIMDS} SIMDs, {CLOCK_GHZ} GHz) {mfma_ms:.3f} ms"
        f" = {100 * mfma_ms / calls['fwd']:.0f} % of the measured time",
        f"  tl_psf_rot_accumulate_bwd  {calls['bwd']:9.3f} ms   {calls['bwd'] * 1e6 / ray_terms:.4f} ns per triple;"
        f" VALU estimate ({valu} VALU + {trans} v_exp_f32 per triple at {ny} x {nxp} padded bins, 4 and 16 cycles per wave) {valu_ms:.3f} ms"
        f" = {100 * valu_ms / calls['bwd']:.0f} % of the measured time",
        "peak growth of torch.cuda.max_memory_allocated over one step:",
        f"  fused        {mem[True] / rays[True]:8.1f} B per ray   ({mem[True] / 2**20:.0f} MiB)",
        f"  fused=False  {mem[False] / rays[False]:8.1f} B per ray   ({mem[False] / 2**20:.0f} MiB)"
        f" = {mem[False] / rays[False] / n_terms * F:.1f} B per ray and term",
        f"workspace of the fused calls: {nbytes} B = {nbytes / rays[True]:.4f} B per ray",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
