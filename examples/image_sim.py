#!/usr/bin/env python3
"""
Image quality as a merit function: render a synthetic chart through the Cooke triplet and pull the rendering towards the chart.

    trace kernels -> metrics.psf_from_trace(fused=True) for a column of fields -> imaging.psf_grid_from_fields (a view)
    -> imaging.svola_convolution of the chart (one PSF per band of image height) -> MSE against the chart

with a few Adam steps on the curvatures and thicknesses.  The focal length is free to drift here (no constraint term): the
point is the chain and its gradient, not a design.

    python examples/image_sim.py --steps 10 [--log2-pupil 12] [--pixel 0.004] [--torch]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chart(h, w, device):
    """Bars of growing frequency, a slanted edge and a few points, RGB in [0, 1]."""
    y, x = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32), torch.arange(w, device=device, dtype=torch.float32),
                          indexing="ij")
    bars = 0.5 + 0.5 * torch.sign(torch.sin(2 * torch.pi * (x / w) ** 2 * w / 6))
    edge = (x - w / 2 > 0.2 * (y - h / 2)).float()
    img = torch.where(y < h / 2, bars, edge)
    img[(y.long() % 16 == 8) & (x.long() % 16 == 8)] = 1.0
    return torch.stack((img, 0.9 * img + 0.05, 1 - 0.8 * img), dim=-1)[None]


def run(steps=10, lr=2e-4, log2_pupil=12, pixel=0.004, n_fields=5, size=(96, 64), n_bins=(9, 9), fused=True, device="cuda:0",
        verbose=False):
    import yaml_free_lenses as L
    import torchoptics_amd as ta
    from torchoptics_amd import imaging, metrics
    lens0, specs, leaves = L.build("cooke", device)
    structure = lens0.structure
    del lens0                                    # keep no autograd graph alive across steps (see adam_loop.py)
    n_r = 1 << (log2_pupil // 2)
    fields = tuple(float(v) for v in torch.linspace(0, 1, n_fields))
    tracer = ta.RayTracer(mode="circular", n_rays=(n_r, (1 << log2_pupil) // n_r), rel_fields=fields, wavelengths=("C", "d", "F"),
                          default_device=device)
    nd, v = leaves["nd"].detach(), leaves["v"].detach()
    opt = torch.optim.Adam([leaves["c"], leaves["t"]], lr=lr)
    target = chart(*size, device)
    history = []
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        lens = ta.Lens(structure, leaves["c"], leaves["t"], nd, v)
        x, y, cx, cy, ok, back = tracer.trace_rays(specs, lens)
        kernels = metrics.psf_from_trace(x, y, ok, n_bins=n_bins, increment=pixel, fused=True)[3]     # [F, W, 9, 9]
        psfs = imaging.psf_grid_from_fields(kernels, (n_fields, 1))                                   # [1, F, 9, 9, W]: a view
        rendered = imaging.svola_convolution(target, 8, psfs, (n_fields, 1), "hann", fused=fused)
        loss = ((rendered - target) ** 2).mean()
        loss.backward()
        opt.step()
        history.append(loss.detach())
    losses = torch.stack(history).cpu().tolist()
    out = dict(workload="cooke", chart=list(size), fields=n_fields, rays_per_step=n_fields * 3 << log2_pupil, steps=steps,
               fused=bool(fused), pixel_mm=pixel, loss_initial=losses[0], loss_final=losses[-1])
    if verbose:
        print(json.dumps(out))
    return out, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--log2-pupil", type=int, default=12)
    ap.add_argument("--pixel", type=float, default=0.004, help="pixel size in mm")
    ap.add_argument("--torch", action="store_true", help="the plain torch formulation of the convolution")
    a = ap.parse_args()
    out, losses = run(a.steps, a.lr, a.log2_pupil, a.pixel, fused=not a.torch, verbose=True)
    if not out["loss_final"] < out["loss_initial"]:
        raise SystemExit("the loss did not fall")


if __name__ == "__main__":
    main()
