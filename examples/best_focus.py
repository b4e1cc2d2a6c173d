#!/usr/bin/env python3
"""
Judging a lens at its best focus: metrics.through_focus on the Cooke triplet.

Prints, from ONE trace, where every field focuses (the shift of the image plane that minimises its RMS spot radius, common to
C, d and F), its tangential and sagittal foci in d, and the on-axis axial colour; then runs a few Adam steps on the curvatures
and thicknesses with the mean over fields of rms_best as the merit function -- the spot size each field would have at its own
best plane, so defocus does not enter the merit and the focal plane may drift without being counted as blur.  Exits non-zero
if rms_best did not fall.

    python examples/best_focus.py [--steps 10] [--log2-pupil 12] [--torch]
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


def run(steps=10, lr=2e-4, log2_pupil=12, fused=None, device="cuda:0", verbose=False):
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
        x, y, cx, cy, ok, back = tracer.trace_rays(specs, lens)
        tf = metrics.through_focus(x, y, cx, cy, ok, common=("wavelength",), fused=fused)
        if report is None:
            with torch.no_grad():
                rows = metrics.through_focus(x, y, cx, cy, ok, common=(), fused=fused)
            report = dict(best_focus=tf.best_focus[0].tolist(), rms=tf.rms[0].tolist(), rms_best=tf.rms_best[0].tolist(),
                          focus_t_d=rows.focus_t[0, :, 1].tolist(), focus_s_d=rows.focus_s[0, :, 1].tolist(),
                          axial_colour=rows.best_focus[0, 0].tolist())
        loss = tf.rms_best.mean()
        loss.backward()
        opt.step()
        history.append(loss.detach())
    history = torch.stack(history).cpu().tolist()
    out = dict(workload="cooke", fields=list(FIELDS), rays_per_step=len(FIELDS) * 3 << log2_pupil, steps=steps,
               rms_best_initial=history[0], rms_best_final=history[-1], **report)
    if verbose:
        print("field   best focus   tangential (d)   sagittal (d)   rms -> rms at best focus   [mm]")
        for i, f in enumerate(FIELDS):
            print(f"{f:5.3f}   {report['best_focus'][i]:+10.4f}   {report['focus_t_d'][i]:+14.4f}   {report['focus_s_d'][i]:+12.4f}   "
                  f"{report['rms'][i]:.4f} -> {report['rms_best'][i]:.4f}")
        print("axial colour on axis (best focus of C, d, F): " + " / ".join(f"{z:+.4f}" for z in report["axial_colour"]) + " mm")
        print(f"mean rms_best {history[0]:.6f} -> {history[-1]:.6f} mm after {steps} Adam steps")
        print(json.dumps(out))
    return out, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--log2-pupil", type=int, default=12)
    ap.add_argument("--torch", action="store_true", help="the moments in plain torch ops (float64) instead of the kernels")
    a = ap.parse_args()
    out, _ = run(a.steps, a.lr, a.log2_pupil, fused=False if a.torch else None, verbose=True)
    return 0 if out["rms_best_final"] < out["rms_best_initial"] else 1


if __name__ == "__main__":
    sys.exit(main())
