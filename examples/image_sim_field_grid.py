#!/usr/bin/env python3
"""
The chart of image_sim.py rendered through a 2-D grid of PSFs, each the traced field PSF turned to its cell's azimuth:

    trace kernels (a column of fields along +y) -> imaging.psf_grid_cells (host geometry, once)
    -> imaging.psf_grid_from_trace(fused=True): one rotated soft histogram per (cell, bracketing field), blended per cell
    -> imaging.svola_convolution of the chart -> MSE against the chart

with a few Adam steps on the curvatures and thicknesses of the Cooke triplet, then the fused PSF grid against fused=False on a
small fan.  The coma flare of every cell points along the cell's own radius, not "up" as with psf_grid_from_fields.

    python examples/image_sim_field_grid.py --steps 5 [--grid 5 5] [--log2-pupil 12] [--pixel 0.004]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def run(steps=5, lr=2e-4, log2_pupil=12, pixel=0.004, n_fields=4, grid=(5, 5), size=(80, 80), n_bins=(9, 9), device="cuda:0",
        verbose=False):
    import yaml_free_lenses as L
    import torchoptics_amd as ta
    from image_sim import chart
    from torchoptics_amd import imaging
    lens0, specs, leaves = L.build("cooke", device)
    structure = lens0.structure
    del lens0
    fields = tuple(float(v) for v in torch.linspace(0, 1, n_fields))
    cells = imaging.psf_grid_cells(size, grid, 8, fields)                   # host geometry: once, outside the loop
    nd, v = leaves["nd"].detach(), leaves["v"].detach()
    opt = torch.optim.Adam([leaves["c"], leaves["t"]], lr=lr)
    target = chart(*size, device)

    def psfs_of(log2_p, fused):
        n_r = 1 << (log2_p // 2)
        tracer = ta.RayTracer(mode="circular", n_rays=(n_r, (1 << log2_p) // n_r), rel_fields=fields, wavelengths=("C", "d", "F"),
                              default_device=device)
        lens = ta.Lens(structure, leaves["c"], leaves["t"], nd, v)
        x, y, cx, cy, ok, back = tracer.trace_rays(specs, lens)
        return imaging.psf_grid_from_trace(x, y, ok, cells, n_bins, pixel, fused=fused)     # [1, gh gw, 9, 9, W]

    history = []
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        rendered = imaging.svola_convolution(target, 8, psfs_of(log2_pupil, True), grid, "hann", fused=True)
        loss = ((rendered - target) ** 2).mean()
        loss.backward()
        opt.step()
        history.append(loss.detach())
    losses = torch.stack(history).cpu().tolist()
    with torch.no_grad():
        a, b = psfs_of(8, True), psfs_of(8, False)
    out = dict(workload="cooke", chart=list(size), grid=list(grid), fields=n_fields, terms=int(cells.src.size),
               rays_per_step=n_fields * 3 << log2_pupil, steps=steps, pixel_mm=pixel, loss_initial=losses[0], loss_final=losses[-1],
               fused_vs_torch_max_abs=float((a - b).abs().max()), psf_peak=float(b.max()))
    if verbose:
        print(json.dumps(out))
    return out, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--log2-pupil", type=int, default=12)
    ap.add_argument("--pixel", type=float, default=0.004, help="pixel size in mm")
    ap.add_argument("--grid", type=int, nargs=2, default=(5, 5))
    a = ap.parse_args()
    out, losses = run(a.steps, a.lr, a.log2_pupil, a.pixel, grid=tuple(a.grid), verbose=True)
    if not out["loss_final"] < out["loss_initial"]:
        raise SystemExit("the loss did not fall")
    if not out["fused_vs_torch_max_abs"] <= 1e-4 * out["psf_peak"]:
        raise SystemExit("the fused PSF grid left the torch definition")


if __name__ == "__main__":
    main()
