"""Kernel arguments for truncations / extensions of the synthetic 20-row prescription (prescriptions.zoom20), shared by
test_gpu_buckets.py and test_gpu_kernel_matrix.py.  Extra rows past 20 are flat air/air dummies with a small gap, which
every ray passes undeviated."""
import torch


def lens_args(ta, n_rows, n_rays=(16, 16), rel_fields=(0., 0.6, 1.)):
    """Kernel arguments for the first `n_rows` rows of zoom20 (n_rows <= 20) or zoom20 + dummies."""
    from torchoptics_amd import prescriptions as P
    lens, specs, leaves = P.zoom20("cpu", requires_grad=False)
    tr = ta.RayTracer(mode="circular", n_rays=n_rays, rel_fields=rel_fields, wavelengths=("C", "d", "F"),
                      default_device="cpu")
    a = tr.assemble(specs, lens)
    S = a["c"].shape[-1]
    if n_rows <= S:
        for k in ("c", "t", "mu", "mask"):
            a[k] = a[k][..., :n_rows].contiguous()
        if n_rows < S:                      # image plane right behind the last kept row
            a["t"] = a["t"].clone()
            a["t"][..., -1] = 0.5
    else:
        extra = n_rows - S
        t_last = a["t"][..., -1:].clone()
        a["c"] = torch.cat((a["c"], torch.zeros(1, 1, 1, 1, extra)), -1)
        a["mu"] = torch.cat((a["mu"], torch.ones(1, 1, 1, a["mu"].shape[3], extra)), -1)
        a["mask"] = torch.cat((a["mask"], torch.ones(1, 1, 1, 1, extra, dtype=torch.bool)), -1)
        gaps = torch.full((1, 1, 1, 1, extra), 0.05)
        a["t"] = torch.cat((a["t"][..., :-1], gaps, t_last - 0.05 * extra), -1)
    return a
