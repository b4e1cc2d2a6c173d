#!/usr/bin/env python3
"""
The rendered sensor image scored the way the reference's renderer scores it (apply_optics_model reports tf.image.ssim and
tf.image.psnr of the blurred image against the input): the chain of examples/image_sim_reference_order.py,

    trace kernels -> metrics.psf_from_trace(fused=True) -> imaging.psf_grid_from_fields -> imaging.svola_convolution(chart) = blurred
    metrics.compute_distortion -> imaging.distortion_grid -> x, y ;  metrics.compute_relative_illumination -> imaging.radial_map -> gain
    imaging.warp_bicubic(blurred, x, y, gain, image_grad="fused") = rendered

ending in the structural similarity as the merit function,  loss = 1 - imaging.ssim(rendered, chart).mean(),  with a few Adam
steps on the curvatures and thicknesses of the Cooke triplet.  SSIM and PSNR are printed before and after.  The focal length is
free to drift (no constraint term): the point is the chain and its gradient, not a design.

    python examples/image_sim_ssim.py --steps 10 [--log2-pupil 12] [--pixel 0.004] [--torch] [--merit ms-ssim] [--graph]

--merit ms-ssim minimises 1 - imaging.ms_ssim instead (tf's weights over as many levels as the chart carries with the 11-tap
window: three for 96 x 64) and prints the MS-SSIM next to SSIM and PSNR.  --torch takes the plain torch formulations of the convolution, the warp and the SSIM instead of the kernels.

--graph records the whole step -- both metric traces, the fan, PSFs, convolution, warp, merit, backward and Adam(capturable=True) --
into a HIP graph (torchoptics_amd.graphs.capture_step) and replays it, after one call of the step on the capture stream under
torch.cuda.set_sync_debug_mode("error"): a step that still synchronises with the host ends there with an exception and is never
captured.  It prints one JSON line with the loss and SSIM of every step run eagerly and of the same number of parameter updates
run as warm-up plus replays; the two trajectories must be equal.
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


def ms_ssim_weights(size, filter_size=11):
    """tf's power factors for as many levels as the chart carries with the window (every level at least filter_size on both
    sides), normalised to sum 1."""
    from torchoptics_amd import imaging
    h, w = size
    m = 0
    while m < len(imaging.MS_SSIM_POWER_FACTORS) and min(h, w) >= filter_size:
        h, w, m = (h + 1) // 2, (w + 1) // 2, m + 1
    p = imaging.MS_SSIM_POWER_FACTORS[:m]
    return tuple(v / sum(p) for v in p)


def make_forward(leaves, structure, specs, device, log2_pupil=12, pixel=0.004, n_fields=5, size=(96, 64), n_bins=(9, 9), fused=True,
                 merit="ssim"):
    """forward() -> (loss, ssim [1], ms_ssim [1] or None, rendered): the chain of this example from the bare leaves c and t
    (`leaves`) to the merit, built anew on every call so that no autograd graph outlives a step.  Everything that is constant
    -- the tracer, the chart, the host tuples of fields -- is made here, once."""
    import torchoptics_amd as ta
    from image_sim import chart
    from torchoptics_amd import imaging, metrics
    n_r = 1 << (log2_pupil // 2)
    fields = tuple(float(v) for v in torch.linspace(0, 1, n_fields))
    tracer = ta.RayTracer(mode="circular", n_rays=(n_r, (1 << log2_pupil) // n_r), rel_fields=fields, wavelengths=("C", "d", "F"),
                          default_device=device)
    nd, v = leaves["nd"].detach(), leaves["v"].detach()
    target = chart(*size, device)
    weights = ms_ssim_weights(target.shape[1:3]) if merit == "ms-ssim" else None

    def forward():
        lens = ta.Lens(structure, leaves["c"], leaves["t"], nd, v)
        d = metrics.compute_distortion(specs, lens, fields[1:], default_device=device)
        ri = metrics.compute_relative_illumination(specs, lens, fields, wavelengths=("C", "d", "F"), default_device=device)
        x, y = imaging.distortion_grid(d, fields[1:], size)
        gain = imaging.radial_map(ri[:, 1:], fields[1:], size, v0=1.0)
        xr, yr, cx, cy, ok, back = tracer.trace_rays(specs, lens)
        kernels = metrics.psf_from_trace(xr, yr, ok, n_bins=n_bins, increment=pixel, fused=True)[3]
        psfs = imaging.psf_grid_from_fields(kernels, (n_fields, 1))
        blurred = imaging.svola_convolution(target, 8, psfs, (n_fields, 1), "hann", fused=fused)
        rendered = imaging.warp_bicubic(blurred, x, y, gain, fused=None if fused else False, image_grad="fused")
        value = imaging.ssim(rendered, target, fused=None if fused else False)
        ms = None
        if merit == "ms-ssim":
            ms = imaging.ms_ssim(rendered, target, power_factors=weights, fused=None if fused else False)
            loss = 1 - ms.mean()
        else:
            loss = 1 - value.mean()
        return loss, value, ms, rendered
    forward.target, forward.weights = target, weights
    return forward


def _cooke(device):
    import yaml_free_lenses as L
    lens0, specs, leaves = L.build("cooke", device)
    structure = lens0.structure
    del lens0                                    # keep no autograd graph alive across steps (see adam_loop.py)
    return structure, specs, leaves


def run(steps=10, lr=2e-4, log2_pupil=12, pixel=0.004, n_fields=5, size=(96, 64), n_bins=(9, 9), fused=True, device="cuda:0",
        verbose=False, merit="ssim"):
    from torchoptics_amd import imaging
    structure, specs, leaves = _cooke(device)
    forward = make_forward(leaves, structure, specs, device, log2_pupil, pixel, n_fields, size, n_bins, fused, merit)
    target, weights = forward.target, forward.weights
    opt = torch.optim.Adam([leaves["c"], leaves["t"]], lr=lr)
    ssims, psnrs, merits = [], [], []
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        loss, value, ms, rendered = forward()
        if ms is not None:
            merits.append(ms.detach().mean())
        loss.backward()
        opt.step()
        ssims.append(value.detach().mean())
        psnrs.append(imaging.psnr(rendered.detach(), target).mean())
    ssims, psnrs = torch.stack(ssims).cpu().tolist(), torch.stack(psnrs).cpu().tolist()
    out = dict(workload="cooke", chart=list(size), fields=n_fields, rays_per_step=n_fields * 3 << log2_pupil, steps=steps,
               fused=bool(fused), pixel_mm=pixel, ssim_initial=ssims[0], ssim_final=ssims[-1], psnr_initial=psnrs[0],
               psnr_final=psnrs[-1])
    if merit == "ms-ssim":
        merits = torch.stack(merits).cpu().tolist()
        out.update(merit="ms-ssim", levels=len(weights), ms_ssim_initial=merits[0], ms_ssim_final=merits[-1])
    if verbose:
        print(json.dumps(out))
    return out, ssims


def run_graph(steps=6, lr=2e-4, log2_pupil=12, pixel=0.004, n_fields=5, size=(96, 64), n_bins=(9, 9), device="cuda:0", merit="ssim",
              verbose=False):
    """`steps` parameter updates twice from the same start, Adam(capturable=True) both times: eagerly, and as three warm-up
    steps on the capture stream (the third under the sync debug mode) plus steps - 3 replays of the recorded step.  Returns the
    two trajectories of (loss, SSIM), one entry per update, each taken before its update."""
    from torchoptics_amd import graphs
    if steps < 4:
        raise ValueError("--graph needs at least 4 steps: three warm up the capture stream, the rest are replays")
    kw = dict(log2_pupil=log2_pupil, pixel=pixel, n_fields=n_fields, size=size, n_bins=n_bins, fused=True, merit=merit)

    def loop():
        structure, specs, leaves = _cooke(device)
        leaves["c"], leaves["t"] = graphs.fresh_leaves(leaves["c"], leaves["t"])
        forward = make_forward(leaves, structure, specs, device, **kw)
        opt = torch.optim.Adam([leaves["c"], leaves["t"]], lr=lr, capturable=True)

        def one_step():
            opt.zero_grad(set_to_none=True)
            loss, value, _, _ = forward()
            loss.backward()
            opt.step()
            return loss.detach(), value.detach().mean()
        return one_step

    step = loop()
    eager = [torch.stack(step()) for _ in range(steps)]
    step = loop()
    history = []
    cap = torch.cuda.Stream(device)
    cap.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(cap):
        history += [torch.stack(step()) for _ in range(2)]
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")          # a step that synchronises with the host raises here: no capture
        try:
            history.append(torch.stack(step()))
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.current_stream(device).wait_stream(cap)
    torch.cuda.synchronize()
    graph, static = graphs.capture_step(step, device, warmup=0, stream=cap)
    for _ in range(steps - 3):
        graph.replay()
        history.append(torch.stack(static))
    torch.cuda.synchronize()
    eager, replayed = torch.stack(eager).cpu(), torch.stack(history).cpu()
    out = dict(workload="cooke", chart=list(size), fields=n_fields, rays_per_step=n_fields * 3 << log2_pupil, steps=steps,
               merit=merit, hip_graph=True, sync_free=True, replays=steps - 3,
               loss_eager=eager[:, 0].tolist(), loss_graph=replayed[:, 0].tolist(),
               ssim_eager=eager[:, 1].tolist(), ssim_graph=replayed[:, 1].tolist())
    if verbose:
        print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--log2-pupil", type=int, default=12)
    ap.add_argument("--pixel", type=float, default=0.004, help="pixel size in mm")
    ap.add_argument("--torch", action="store_true", help="the plain torch formulations of the convolution, the warp and the SSIM")
    ap.add_argument("--merit", choices=("ssim", "ms-ssim"), default="ssim",
                    help="the merit function Adam minimises 1 minus: imaging.ssim or imaging.ms_ssim (as many of tf's levels as the chart carries)")
    ap.add_argument("--fields", type=int, default=5, help="fields traced along the meridian, one PSF band each")
    ap.add_argument("--size", type=int, nargs=2, default=(96, 64), metavar=("H", "W"), help="the chart's rows and columns")
    ap.add_argument("--graph", action="store_true",
                    help="record the whole step with Adam(capturable=True) into a HIP graph, replay it and compare with the eager loop")
    a = ap.parse_args()
    if a.graph:
        if a.torch:
            raise SystemExit("--graph records the kernels' step: it does not go with --torch")
        out = run_graph(a.steps, a.lr, a.log2_pupil, a.pixel, a.fields, tuple(a.size), merit=a.merit, verbose=True)
        if out["loss_graph"] != out["loss_eager"] or out["ssim_graph"] != out["ssim_eager"]:
            raise SystemExit("the replayed trajectory is not the eager one")
        if not out["loss_graph"][-1] != out["loss_graph"][0]:
            raise SystemExit("the loss did not move")
        print(f"{a.steps} updates, {out['replays']} of them replayed from a HIP graph: loss {out['loss_graph'][0]:.6f} -> "
              f"{out['loss_graph'][-1]:.6f}, the eager loop's bits")
        return
    out, _ = run(a.steps, a.lr, a.log2_pupil, a.pixel, a.fields, tuple(a.size), fused=not a.torch, verbose=True, merit=a.merit)
    if a.merit == "ms-ssim":
        print(f"MS-SSIM ({out['levels']} levels) {out['ms_ssim_initial']:.6f} -> {out['ms_ssim_final']:.6f}")
    print(f"SSIM {out['ssim_initial']:.6f} -> {out['ssim_final']:.6f}, PSNR {out['psnr_initial']:.3f} dB -> {out['psnr_final']:.3f} dB")
    if a.merit == "ms-ssim":
        if not out["ms_ssim_final"] > out["ms_ssim_initial"]:
            raise SystemExit("the MS-SSIM did not rise")
    elif not out["ssim_final"] > out["ssim_initial"]:
        raise SystemExit("the SSIM did not rise")


if __name__ == "__main__":
    main()
