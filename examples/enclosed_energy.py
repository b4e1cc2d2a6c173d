#!/usr/bin/env python3
"""
The enclosed-energy curve of a lens and the radius that holds 80 % of the light: metrics.enclosed_energy / enclosed_radius on
the Cooke triplet.

Prints, from ONE trace, the encircled energy of every field (C, d and F pooled, each wavelength about its own centroid) at 16
radii and the 80 % radius, then runs a few Adam steps on the curvatures and thicknesses with the mean 80 % radius as the merit
function -- the figure most specifications are written in.  The smooth edge of the definition (half width `--softness`) is what
gives that merit a gradient.  Exits non-zero if the mean 80 % radius did not fall.

    python examples/enclosed_energy.py [--steps 10] [--log2-pupil 12] [--square] [--torch]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = (0.0, 0.5, 0.707, 1.0)
LINES = ("C", "d", "F")
RADII = tuple(0.008 * k for k in range(1, 17))          # mm


def run(steps=10, lr=1e-4, log2_pupil=12, shape="circle", softness=0.004, fused=None, device="cuda:0", verbose=False):
    import yaml_free_lenses as L
    import torchoptics_amd as ta
    from torchoptics_amd import metrics
    lens0, specs, leaves = L.build("cooke", device)
    structure = lens0.structure
    del lens0                                    # keep no autograd graph alive across steps (see adam_loop.py)
    n_r = 1 << (log2_pupil // 2)
    tracer = ta.RayTracer(mode="circular", n_rays=(n_r, (1 << log2_pupil) // n_r), rel_fields=FIELDS, wavelengths=LINES,
                          default_device=device)
    nd, v = leaves["nd"].detach(), leaves["v"].detach()
    opt = torch.optim.Adam([leaves["c"], leaves["t"]], lr=lr)
    history, report = [], None
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        lens = ta.Lens(structure, leaves["c"], leaves["t"], nd, v)
        x, y, _, _, ok, _ = tracer.trace_rays(specs, lens)
        e = metrics.enclosed_energy(x, y, ok, RADII, softness, shape=shape, common=("wavelength",), fused=fused)
        r80, reached = metrics.enclosed_radius(e.energy, RADII, 0.8)
        if report is None:
            report = dict(energy=e.energy[0].tolist(), r80=r80[0].tolist(), reached=reached[0].tolist())
        loss = r80.mean()
        loss.backward()
        opt.step()
        history.append(loss.detach())
    history = torch.stack(history).cpu().tolist()
    out = dict(workload="cooke", shape=shape, fields=list(FIELDS), radii=list(RADII), softness=softness,
               rays_per_step=len(FIELDS) * 3 << log2_pupil, steps=steps, lr=lr, r80_initial=history[0], r80_final=history[-1],
               r80_history=history, **report)
    if verbose:
        print(f"{'en' + shape + 'd'} energy, C + d + F; radius [mm]: " + " ".join(f"{r:5.3f}" for r in RADII))
        for i, f in enumerate(FIELDS):
            print(f"field {f:5.3f}                         " + " ".join(f"{v:5.3f}" for v in report["energy"][i])
                  + f"   80 % inside {report['r80'][i]:.4f} mm" + ("" if report["reached"][i] else " (not reached)"))
        print(f"mean 80 % radius {history[0]:.6f} -> {history[-1]:.6f} mm after {steps} Adam steps")
        print(json.dumps(out))
    return out, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--log2-pupil", type=int, default=12)
    ap.add_argument("--softness", type=float, default=0.004)
    ap.add_argument("--square", action="store_true", help="ensquared energy: the radii are half sides of a pixel")
    ap.add_argument("--torch", action="store_true", help="the sums in plain torch ops (float64) instead of the kernels")
    a = ap.parse_args()
    out, _ = run(a.steps, a.lr, a.log2_pupil, "square" if a.square else "circle", a.softness, fused=False if a.torch else None,
                 verbose=True)
    return 0 if out["r80_final"] < out["r80_initial"] else 1


if __name__ == "__main__":
    sys.exit(main())
