#!/usr/bin/env python3
"""
The wavefront of a lens from its spot: metrics.zernike_fit on the Cooke triplet.

Prints, per field at the d line, the Zernike coefficients Z4 .. Z11 (Noll) in waves -- defocus, the two astigmatisms, the two
comas, the two trefoils and spherical -- with the RMS wavefront error without tilt, and without tilt and defocus, all from the
transverse ray errors of ONE trace (no optical path length is computed); then runs a few Adam steps on the curvatures and
thicknesses with the mean over fields and wavelengths of rms_focus as the merit function.  Exits non-zero if it did not fall.

    python examples/wavefront_fit.py [--steps 10] [--log2-pupil 12] [--order 4] [--torch]
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
NM = (656.3, 587.6, 486.1)


def run(steps=10, lr=2e-4, log2_pupil=12, order=4, fused=None, device="cuda:0", verbose=False):
    import yaml_free_lenses as L
    import torchoptics_amd as ta
    from torchoptics_amd import metrics, paraxial
    lens0, specs, leaves = L.build("cooke", device)
    structure = lens0.structure
    del lens0                                    # keep no autograd graph alive across steps (see adam_loop.py)
    n_r = 1 << (log2_pupil // 2)
    tracer = ta.RayTracer(mode="circular", n_rays=(n_r, (1 << log2_pupil) // n_r), rel_fields=FIELDS, wavelengths=LINES,
                          default_device=device)
    nd, v = leaves["nd"].detach(), leaves["v"].detach()
    lam = torch.tensor(NM, device=device) * 1e-6                               # mm, as x and y
    opt = torch.optim.Adam([leaves["c"], leaves["t"]], lr=lr)
    history, report = [], None
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        lens = ta.Lens(structure, leaves["c"], leaves["t"], nd, v)
        x, y, cx, cy, ok, back = tracer.trace_rays(specs, lens)
        px, py = tracer.pupil_coordinates(specs, lens)
        # an object at infinity: W = (epd / 2 efl) a, in waves of every row's own wavelength (differentiable through the efl)
        scale = (specs.epd / (2 * paraxial.get_first_order(lens)[0])).reshape(-1, 1, 1) / lam
        fit = metrics.zernike_fit(x, y, ok, px, py, max_order=order, scale=scale, fused=fused)
        if report is None:
            report = dict(coeffs_d=fit.coeffs[0, :, 1, 2:10].detach().tolist(), rms_d=fit.rms[0, :, 1].detach().tolist(),
                          rms_focus_d=fit.rms_focus[0, :, 1].detach().tolist(), valid=bool(fit.valid.all()))
        loss = fit.rms_focus.mean()
        loss.backward()
        opt.step()
        history.append(loss.detach())
    history = torch.stack(history).cpu().tolist()
    out = dict(workload="cooke", fields=list(FIELDS), order=order, rays_per_step=len(FIELDS) * 3 << log2_pupil, steps=steps,
               rms_focus_initial=history[0], rms_focus_final=history[-1], **report)
    if verbose:
        print("field  " + "".join(f"{'Z' + str(j):>9s}" for j in range(4, 12)) + "      rms   rms less focus   [waves at d]")
        for i, f in enumerate(FIELDS):
            print(f"{f:5.3f}  " + "".join(f"{c:+9.4f}" for c in report["coeffs_d"][i])
                  + f"   {report['rms_d'][i]:.4f}   {report['rms_focus_d'][i]:.4f}")
        print(f"mean rms_focus {history[0]:.6f} -> {history[-1]:.6f} waves after {steps} Adam steps")
        print(json.dumps(out))
    return out, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--log2-pupil", type=int, default=12)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--torch", action="store_true", help="the fit in plain torch ops (float64) instead of the kernels")
    a = ap.parse_args()
    out, _ = run(a.steps, a.lr, a.log2_pupil, a.order, fused=False if a.torch else None, verbose=True)
    return 0 if out["rms_focus_final"] < out["rms_focus_initial"] else 1


if __name__ == "__main__":
    sys.exit(main())
