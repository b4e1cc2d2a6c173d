#!/usr/bin/env python3
"""
MTF against focus shift: metrics.through_focus_mtf on the Cooke triplet.

Prints, from ONE trace, the polychromatic (C, d, F) MTF at 20 and 40 cycles / mm, tangential and sagittal, at 16 image planes over
+-0.15 mm per field, and the MTF-best focus at 40 cycles / mm (metrics.mtf_best_focus) next to the RMS-best focus of
metrics.through_focus; then runs a few Adam steps on the curvatures and thicknesses with minus the mean over fields of the
tangential and sagittal peak MTF at 40 cycles / mm as the merit function -- the MTF each field would have at its own best
plane.  Exits non-zero if the peak MTF did not rise.

    python examples/through_focus_mtf.py [--steps 10] [--log2-pupil 12] [--torch]
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
FREQUENCIES = (20.0, 40.0)
PLANES = (-0.15, 0.02, 16)


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
        tf = metrics.through_focus_mtf(x, y, cx, cy, ok, FREQUENCIES, PLANES, fused=fused)          # mtf [1, F, Z, 2, 2]
        shift, peak, interior = metrics.mtf_best_focus(tf.mtf, tf.shifts)                           # [1, F, 2, 2]
        if report is None:
            with torch.no_grad():
                rms = metrics.through_focus(x, y, cx, cy, ok, common=("wavelength",), fused=fused)
            report = dict(shifts=tf.shifts.tolist(), mtf=tf.mtf[0].tolist(), mtf_best_focus_40=shift[0, :, :, 1].tolist(),
                          mtf_peak_40=peak[0, :, :, 1].tolist(), interior_40=interior[0, :, :, 1].tolist(),
                          rms_best_focus=rms.best_focus[0].tolist())
        merit = peak[..., 1].mean()                                                                  # T and S at 40 cycles / mm
        (-merit).backward()
        opt.step()
        history.append(merit.detach())
    history = torch.stack(history).cpu().tolist()
    out = dict(workload="cooke", fields=list(FIELDS), rays_per_step=len(FIELDS) * 3 << log2_pupil, steps=steps,
               peak_mtf_40_initial=history[0], peak_mtf_40_final=history[-1], **report)
    if verbose:
        for i, f in enumerate(FIELDS):
            print(f"field {f:5.3f}   shift [mm]  " + "  ".join(f"{d:+6.2f}" for d in report["shifts"]))
            for d, name in enumerate("TS"):
                for k, nu in enumerate(FREQUENCIES):
                    print(f"   {name} {nu:4.0f} cycles/mm      " + "  ".join(f"{report['mtf'][i][z][d][k]:6.3f}" for z in range(PLANES[2])))
        print("field   MTF-best focus at 40 cycles/mm T / S (peak MTF)           RMS-best focus   [mm]")
        for i, f in enumerate(FIELDS):
            t, s = report["mtf_best_focus_40"][i]
            pt, ps = report["mtf_peak_40"][i]
            edge = "" if all(report["interior_40"][i]) else "   (a maximum on the first or last plane)"
            print(f"{f:5.3f}   {t:+8.4f} ({pt:.3f}) / {s:+8.4f} ({ps:.3f})                       {report['rms_best_focus'][i]:+8.4f}{edge}")
        print(f"mean peak MTF at 40 cycles/mm {history[0]:.4f} -> {history[-1]:.4f} after {steps} Adam steps")
        print(json.dumps({k: v for k, v in out.items() if k != "mtf"}))
    return out, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--log2-pupil", type=int, default=12)
    ap.add_argument("--torch", action="store_true", help="the sums in plain torch ops (float64) instead of the kernels")
    a = ap.parse_args()
    out, _ = run(a.steps, a.lr, a.log2_pupil, fused=False if a.torch else None, verbose=True)
    return 0 if out["peak_mtf_40_final"] > out["peak_mtf_40_initial"] else 1


if __name__ == "__main__":
    sys.exit(main())
