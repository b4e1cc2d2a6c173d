"""The steps that are held to their eager bits on a side stream, under the sync debug mode and from a HIP graph
(tests/test_gpu_steps_graph.py), and, where they have a torch path, twice on the CPU (tests/test_steps_cpu.py): the imaging and
focus nodes that came after the trace kernels, one step each, and the loops of examples/ made of them.

`build(name, device, fused)` returns a Case:

  leaves   {name: tensor}: fresh leaves (graphs.fresh_leaves: no AccumulateGrad node yet) holding input set A;
  step()   self-contained in the sense of graphs.capture_step: it drops the leaves' gradients, builds its autograd graph from the
           bare leaves, calls backward and returns the tensors to read -- the outputs (`outputs` names them), then the gradient
           of every leaf in `grads`;
  sets     {"A": {leaf: CPU tensor}, "B": ...}: two seeded input sets, float32 values as they stand (nothing is rounded on
           the way to the device); load("B") writes one into the leaves with copy_;
  counters the ops.*_counts functions of the nodes in the step that keep one.

Every constant of a step -- seeds of the backward, masks, the chart, the tracer, host tuples of fields -- is made by the
builder, not by the step: a step reads leaves and constants and uploads nothing.

Shapes are the issue's: the smallest that still reach a second tile or block and a short tail.  Nothing had to be adjusted for
an argument check.  "image_sim" takes the smallest sizes the chain's checks accept: 3 fields, a 48 x 32 chart (two MS-SSIM
levels under the 11-tap window), overlap 8, 2^8 rays per field and wavelength.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "examples")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


class Case:
    def __init__(self, device, sets, body, outputs, grads, counters=()):
        from torchoptics_amd import graphs
        self.device, self.sets, self.outputs, self.grads, self.counters = device, sets, tuple(outputs), tuple(grads), tuple(counters)
        self.leaves = {k: graphs.fresh_leaves(v.to(device)) for k, v in sets["A"].items()}
        self._body = body

    @property
    def names(self):
        return self.outputs + tuple("d/d" + g for g in self.grads)

    def step(self):
        for t in self.leaves.values():
            t.grad = None
        outs = self._body(self.leaves)
        return tuple(o.detach() for o in outs) + tuple(self.leaves[g].grad for g in self.grads)

    def load(self, which):
        with torch.no_grad():
            for k, v in self.sets[which].items():
                self.leaves[k].copy_(v)

    def counts(self):
        """The integer call counters of the step's nodes (the pointers they also record are left out)."""
        return {f.__name__ + "." + k: v for f in self.counters for k, v in f().items() if not k.endswith("_ptr")}


def _uniform(rng, shape, lo=0.0, hi=1.0):
    return torch.from_numpy((lo + (hi - lo) * rng.random(shape)).astype(np.float32))


def _normal(rng, shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32))


def _tracer_layout(a):
    """[B,F,W,P] numpy -> the tracer's [B,F,P,W] view of that memory, float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).permute(0, 1, 3, 2)


def _svola(device, fused):
    from torchoptics_amd import imaging, ops
    rng = np.random.default_rng(101)
    sets = {w: dict(image=_uniform(rng, (2, 24, 40, 3)), psfs=_uniform(rng, (2, 4, 5, 5, 3))) for w in "AB"}
    seed = _normal(rng, (2, 24, 40, 3)).to(device)

    def body(L):
        out = imaging.svola_convolution(L["image"], 4, L["psfs"], (2, 2), "hann", fused=fused)
        (out * seed).sum().backward()
        return (out,)
    return Case(device, sets, body, ("out",), ("image", "psfs"), (ops.svola_counts,))


def _warp(path):
    def build(device, fused):
        from torchoptics_amd import imaging, ops
        rng = np.random.default_rng(202)
        sets = {w: dict(image=_uniform(rng, (2, 20, 24, 3)), x=_uniform(rng, (1, 17, 33), -1.1, 1.1),
                        y=_uniform(rng, (1, 17, 33), -1.1, 1.1), gain=_uniform(rng, (1, 17, 33, 1), 0.5, 1.5)) for w in "AB"}
        seed = _normal(rng, (2, 17, 33, 3)).to(device)

        def body(L):
            ops.set_warp_image_grad_path(path)              # read by the image backward; host state, nothing is launched
            try:
                out = imaging.warp_bicubic(L["image"], L["x"], L["y"], L["gain"], fused=fused, image_grad="fused")
                (out * seed).sum().backward()
            finally:
                ops.set_warp_image_grad_path("auto")
            return (out,)
        return Case(device, sets, body, ("out",), ("x", "y", "gain", "image"), (ops.warp_counts,))
    return build


def _image_pair(rng, shape):
    a = rng.random(shape)
    return dict(a=torch.from_numpy(a.astype(np.float32)),
                b=torch.from_numpy(np.clip(a + 0.1 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)))


def _ssim(shape, K):
    def build(device, fused):
        from torchoptics_amd import imaging, ops
        rng = np.random.default_rng(303 + K)
        sets = {w: _image_pair(rng, shape) for w in "AB"}
        seed = torch.tensor([1.0, -0.5][:shape[0]]).to(device)

        def body(L):
            value = imaging.ssim(L["a"], L["b"], filter_size=K, fused=fused)
            (value * seed).sum().backward()
            return (value,)
        return Case(device, sets, body, ("ssim",), ("a", "b"), (ops.ssim_counts,))
    return build


def _ms_ssim(device, fused):
    from torchoptics_amd import imaging, ops
    rng = np.random.default_rng(404)
    sets = {w: _image_pair(rng, (2, 21, 37, 3)) for w in "AB"}
    seed = torch.tensor([1.0, -0.5]).to(device)
    p = imaging.MS_SSIM_POWER_FACTORS[:3]
    power = tuple(v / sum(p) for v in p)

    def body(L):
        value, terms = imaging.ms_ssim(L["a"], L["b"], power_factors=power, filter_size=5, fused=fused, return_terms=True)
        (value * seed).sum().backward()
        return value, terms
    return Case(device, sets, body, ("ms_ssim", "terms"), ("a", "b"), (ops.ms_ssim_counts,))


def _focus(device, fused):
    import focus_cases
    from torchoptics_amd import metrics
    rays = focus_cases.rays("block-edge")                       # F = 3, W = 2, P = 257
    rng = np.random.default_rng(505)
    keys = ("x", "y", "cx", "cy")
    A = {k: _tracer_layout(rays[k].transpose(0, 1, 3, 2)) for k in keys}
    B = {k: _tracer_layout((rays[k] + 1e-3 * rng.standard_normal(rays[k].shape)).transpose(0, 1, 3, 2)) for k in keys}
    ok = _tracer_layout(rays["ok"].transpose(0, 1, 3, 2)).to(torch.bool).to(device)

    def body(L):
        tf = metrics.through_focus(L["x"], L["y"], L["cx"], L["cy"], ok, common=("wavelength",), fused=fused)
        (tf.rms_best.sum() + tf.best_focus.sum()).backward()
        return tf.rms_best, tf.best_focus
    return Case(device, {"A": A, "B": B}, body, ("rms_best", "best_focus"), keys)


def _psf_grid(device, fused):
    from torchoptics_amd import imaging, ops
    rng = np.random.default_rng(606)
    centre = np.array([0.0, 2.0, 4.0]).reshape(1, 3, 1, 1)

    def fan():
        return dict(x=_tracer_layout(0.008 * rng.standard_normal((1, 3, 3, 300))),
                    y=_tracer_layout(centre + 0.008 * rng.standard_normal((1, 3, 3, 300))))
    sets = {w: fan() for w in "AB"}
    ok = _tracer_layout(rng.random((1, 3, 3, 300)) > 0.1).to(torch.bool).to(device)
    cells = imaging.psf_grid_cells((24, 40), (2, 3), 4, (0.0, 0.6, 1.0))
    image = _uniform(rng, (1, 24, 40, 3)).to(device)
    seed = _normal(rng, (1, 24, 40, 3)).to(device)

    def body(L):
        psfs = imaging.psf_grid_from_trace(L["x"], L["y"], ok, cells, (9, 9), 0.004, fused=fused)
        out = imaging.svola_convolution(image, 4, psfs, (2, 3), "hann", fused=fused)
        (out * seed).sum().backward()
        return psfs, out
    return Case(device, sets, body, ("psfs", "out"), ("x", "y"), (ops.svola_counts,))


def _cooke_sets(rng):
    import yaml_free_lenses as L
    d = L.PRESCRIPTIONS["cooke"]
    c, t = np.asarray(d["c"], dtype=np.float32), np.asarray(d["t"], dtype=np.float32)
    return {"A": dict(c=torch.from_numpy(c), t=torch.from_numpy(t)),
            "B": dict(c=torch.from_numpy((c + 1e-4 * rng.standard_normal(c.shape)).astype(np.float32)),
                      t=torch.from_numpy((t * (1 + 1e-3 * rng.standard_normal(t.shape))).astype(np.float32)))}


def _maps(device, fused):
    import yaml_free_lenses as L
    import torchoptics_amd as ta
    from torchoptics_amd import imaging, metrics
    if not fused:
        raise ValueError("maps: the metrics trace rays, and the tracer has no torch path")
    rng = np.random.default_rng(707)
    lens0, specs, lv = L.build("cooke", device)
    structure = lens0.structure
    del lens0                                                    # keep no autograd graph alive across steps
    nd, v = lv["nd"].detach(), lv["v"].detach()
    fields, size = (0.0, 0.4, 0.7, 1.0), (24, 40)                # host tuples: checked on the host, their device copies cached
    seeds = [_normal(rng, (1, 24, 40)).to(device) for _ in range(2)] + [_normal(rng, (1, 24, 40, 3)).to(device)]

    def body(Lv):
        lens = ta.Lens(structure, Lv["c"], Lv["t"], nd, v)
        d = metrics.compute_distortion(specs, lens, fields[1:], default_device=device)
        ri = metrics.compute_relative_illumination(specs, lens, fields, wavelengths=("C", "d", "F"), default_device=device)
        x, y = imaging.distortion_grid(d, fields[1:], size)
        gain = imaging.radial_map(ri[:, 1:], fields[1:], size, v0=1.0)
        ((x * seeds[0]).sum() + (y * seeds[1]).sum() + (gain * seeds[2]).sum()).backward()
        return x, y, gain
    return Case(device, _cooke_sets(rng), body, ("x", "y", "gain"), ("c", "t"))


def _image_sim(merit):
    def build(device, fused):
        import image_sim_ssim
        from torchoptics_amd import ops
        if not fused:
            raise ValueError("image_sim: the chain traces rays, and the tracer has no torch path")
        structure, specs, lv = image_sim_ssim._cooke(device)
        sets = _cooke_sets(np.random.default_rng(808))
        leaves = dict(nd=lv["nd"], v=lv["v"])                     # c and t are the Case's leaves, put in by every step
        forward = image_sim_ssim.make_forward(leaves, structure, specs, device, log2_pupil=8, n_fields=3, size=(48, 32),
                                              fused=True, merit=merit)

        def body(Lv):
            leaves.update(c=Lv["c"], t=Lv["t"])
            loss, value, ms, rendered = forward()
            loss.backward()
            return (loss, value, rendered) if ms is None else (loss, value, ms, rendered)
        outputs = ("loss", "ssim", "rendered") if merit == "ssim" else ("loss", "ssim", "ms_ssim", "rendered")
        counters = (ops.svola_counts, ops.warp_counts, ops.ssim_counts) + ((ops.ms_ssim_counts,) if merit == "ms-ssim" else ())
        return Case(device, sets, body, outputs, ("c", "t"), counters)
    return build


BUILDERS = {
    "svola": _svola,
    "warp-auto": _warp("auto"),
    "warp-direct": _warp("direct"),
    "ssim-27x43x4-k11": _ssim((1, 27, 43, 4), 11),
    "ssim-20x40x2-k5": _ssim((2, 20, 40, 2), 5),
    "ms_ssim": _ms_ssim,
    "focus": _focus,
    "psf_grid": _psf_grid,
    "maps": _maps,
    "image_sim-ssim": _image_sim("ssim"),
    "image_sim-ms-ssim": _image_sim("ms-ssim"),
}
TORCH_PATH = ("svola", "warp-auto", "ssim-27x43x4-k11", "ssim-20x40x2-k5", "ms_ssim", "focus", "psf_grid")     # run on the CPU too
WORKSPACE = ("warp-auto", "warp-direct", "ssim-27x43x4-k11", "ssim-20x40x2-k5", "ms_ssim", "focus", "psf_grid", "maps",
             "image_sim-ssim", "image_sim-ms-ssim")                                     # steps whose kernels use ops._workspace


def build(name, device, fused):
    return BUILDERS[name](device, fused)
