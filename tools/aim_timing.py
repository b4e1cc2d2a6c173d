#!/usr/bin/env python3
"""
Time of the ray-aiming kernels: tl_ray_aim (one Newton step, one thread per (lens, field, wavelength), 1 + 9 traces in
series) against tl_ray_aim_iter (one 16-lane group per (lens, field, wavelength), 1 + N traces of latency) at
N = 1, 2, 4, 8, on two shapes:
  cooke      B = 1,   F = 3, W = 3  (the reference caller's Cooke triplet)
  minibatch  B = 256, F = 8, W = 3  (examples/minibatch_loss.py: padded perturbed Cooke triplets)

    python tools/aim_timing.py [--launches 200] [--warmup 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/aim_timing.py
    python tools/aim_timing.py --summarize OUT/.../*_kernel_trace.csv     # the table committed under profiles/

Every configuration is launched `warmup + launches` times back to back, in the order printed; the summary splits the
trace's aiming dispatches in that order and reports the median over the timed ones.  Without a profiler the same
configurations are timed by device events (median of per-launch times).  Development tool, not part of the product.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

SHAPES = ("cooke", "minibatch")
CONFIGS = ((None, "tl_ray_aim"), (1, "tl_ray_aim_iter N=1"), (2, "tl_ray_aim_iter N=2"), (4, "tl_ray_aim_iter N=4"),
           (8, "tl_ray_aim_iter N=8"))


def _problem(shape, dev):
    import torchoptics_amd as ta
    if shape == "cooke":
        import yaml_free_lenses as L
        lens, specs, _ = L.build("cooke", dev, grad=False)
        fields, wl = (0., 0.707, 1.), ("C", "d", "F")
    else:
        import minibatch_loss as mb
        st, specs, leaves, _ = mb.build_batch(256, dev)
        lens = ta.Lens(st, *(leaves[k].detach() for k in ("c", "t", "nd", "v")))
        fields, wl = mb.FIELDS, mb.WAVELENGTHS
    return ta.RayTracer(mode="circular", n_rays=(8, 8), rel_fields=fields, wavelengths=wl, default_device=dev), specs, lens


def _launcher(tr, specs, lens, n_iter):
    """A closure that launches one aiming kernel on the current stream (arguments built once)."""
    import torch
    from torchoptics_amd import _lib, ops
    from torchoptics_amd.lens_modeling import const_tensor
    from torchoptics_amd.paraxial import compute_pupil_position
    from torchoptics_amd.ray_tracing import _LINES, _dense
    specs2, front = specs.up_to_stop(), lens.up_to_stop()
    B, K = front.c.shape
    F, W = len(tr.rel_fields), len(tr.wavelengths)
    dev = front.c.device
    with torch.no_grad():
        n = _dense(front.get_refractive_indices(tr.wavelengths))
        n_d = _dense(front.get_refractive_indices([_LINES["d"]]))
        z = _dense(compute_pupil_position(lens, tr.arith, front=front))
    c, t = _dense(front.c), _dense(front.t)
    mask = _dense(front.structure.mask_torch.view(torch.uint8))
    fields = const_tensor(list(tr.rel_fields), torch.float32, dev)
    hfov, epd = _dense(specs2.hfov.float()), _dense(specs2.epd.float())
    out = torch.empty((3, B, F, W), dtype=torch.float32, device=dev)
    P = _lib.ptr
    head = (dev.index, B, F, W, K, P(c), P(t), P(n), P(n_d), P(mask), None, None, None, P(z), P(hfov), P(fields), P(epd), 1)
    tail = (P(out[0]), P(out[1]), P(out[2]), ops._stream_ptr(dev))
    lib = _lib.lib()
    if n_iter is None:
        return lambda: _lib.check(lib.tl_ray_aim(*head, *tail), "tl_ray_aim")
    return lambda: _lib.check(lib.tl_ray_aim_iter(*head, n_iter, None, None, *tail), "tl_ray_aim_iter")


def run(launches, warmup):
    import torch
    dev = torch.device("cuda:0")
    rows = []
    for shape in SHAPES:
        tr, specs, lens = _problem(shape, dev)
        for n_iter, label in CONFIGS:
            launch = _launcher(tr, specs, lens, n_iter)
            for _ in range(warmup):
                launch()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
            for a, b in ev:
                a.record()
                launch()
                b.record()
            torch.cuda.synchronize()
            us = [a.elapsed_time(b) * 1e3 for a, b in ev]
            row = dict(shape=shape, kernel=label, launches=launches, median_us=round(statistics.median(us), 2),
                       min_us=round(min(us), 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def summarize(path, launches, warmup):
    """The aiming dispatches of a rocprofv3 kernel trace, split in launch order into the configurations above."""
    with open(path) as f:
        recs = [r for r in csv.DictReader(f) if "ray_aim" in r["Kernel_Name"]]
    recs.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = warmup + launches
    want = len(SHAPES) * len(CONFIGS) * per
    if len(recs) != want:
        raise SystemExit(f"{path}: {len(recs)} aiming dispatches, expected {want}")
    print(f"{'shape':<10} {'kernel':<22} {'launches':>8} {'median_us':>10} {'min_us':>8}")
    i = 0
    for shape in SHAPES:
        for n_iter, label in CONFIGS:
            chunk = recs[i + warmup:i + per]
            name = "ray_aim_kernel" if n_iter is None else "ray_aim_iter_kernel"
            assert all(name + "(" in r["Kernel_Name"] for r in chunk), label
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk]
            print(f"{shape:<10} {label:<22} {len(us):>8} {statistics.median(us):>10.2f} {min(us):>8.2f}")
            i += per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--summarize", default=None, help="a rocprofv3 *_kernel_trace.csv of a run with the same counts")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.launches, a.warmup)
    else:
        run(a.launches, a.warmup)


if __name__ == "__main__":
    main()
