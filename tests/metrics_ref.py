"""
CPU restatement of the three image-quality metrics of torchoptics_amd/metrics.py -- compute_distortion,
compute_relative_illumination, compute_ray_aiming_error -- the checker of tests/test_gpu_metrics_matrix.py.  Written from the
definitions in their docstrings; nothing here calls torchoptics_amd.metrics or torchoptics_amd.paraxial.

What it is made of:

  inputs     the padded rows of a CPU fp32 Lens / Specs pair (c, t, nd, v, kappa, poly, masks, stop, epd, hfov, vignetting
             factors), widened to `dtype`; the field sines are the correctly rounded fp32 sines of the fp32 angle, as the
             tracer feeds them to its kernels (aim_iter_ref.raw_inputs does the same)
  indices    n(lambda) = A + B / lambda^2 from nd and the Abbe number, air rows 1 (Lens.get_refractive_indices' docstring)
  pupil      z = B / A of the ordered left-to-right product of the row matrices in front of the stop (pupil_ref.fast64's
             chain, here in torch and attached to the graph: the metrics differentiate z)
  aiming     aim_iter_ref.aim on aim_iter_ref.inputs, detached, with tee_ref under a vignetting function and rs in
             'paraxial' mode; the map is rounded to fp32 once, as tl_ray_aim_iter writes it, and applied as
             aim_iter_ref.aimed_fan applies it, clamp(remap(.), -2, 2) epd / 2 (written out here: aimed_fan takes one fan
             shared by all fields, a vignetted fan differs per field)
  trace      oracle.trace_oracle.trace_skew_general under torch autograd (aspheric lenses one at a time)
  EFL, BFL   a fresh left-to-right 2 x 2 product with the last gap zeroed: EFL = -1 / C, BFL = -A / C
  formulas   distortion          d = (y - y_ref) / y_ref, y_ref = EFL tan(field) + (t_last - BFL) cy / sqrt(1 - cy^2), chief
                                 ray, d line
             illumination        (cy_upper - cy_lower) cx_sagittal / max(2 cy_upper(axis, first wavelength)^2, 1e-6); a field
                                 with a dead ray, or whose wavelength has a dead ray on axis, reports exactly 1
             aiming error        y_stop / r_stop - y_pupil of the lower and upper meridional ray on the rows in front of the
                                 stop, y_pupil the vignetted relative height; r_stop the on-axis d-line marginal ray ('real')
                                 or A epd / 2 of the front's ABCD product with its gaps ('paraxial'); the integer 0 when
                                 every stop is row 0

`dtype` is the one switch between the fp64 restatement and its fp32 twin (fp32 inputs, fp32 arithmetic, IEEE square roots):
the twin's distance from fp64 is the noise that sets the gates of tests/metrics_cases.py.  The aiming map is the same in
both (fp64 inside, rounded to fp32): the kernels compute it that way.

`wrong` names a deliberately wrong restatement (WRONG), for the sharpness test of the gates.

The vignetting function is the linear one, vig_fn(fields, v) = fields * v[:, None], with the factors of the Specs.
"""
import numpy as np
import torch

import aim_iter_ref as AR
from oracle.trace_oracle import trace_skew_general

LINES = {"C": 656.3, "d": 587.6, "F": 486.1}
WRONG = ("no-defocus", "last-gap-in", "sin-for-tan", "per-wavelength-axis", "sagittal-cy", "swap-upper-lower", "f-line",
         "unvignetted-height", "z-detached", "neighbour-last")
LEAVES = ("c", "t", "nd", "v", "kappa", "poly")


def linear_vig(fields, v):
    """The vignetting function of the cases: the factor grows linearly with the relative field."""
    return fields * v[:, None]


class System:
    """The rows of a CPU Lens / Specs pair in `dtype`; c, t, nd, v (kappa, poly) are leaves of the graph."""

    def __init__(self, lens, specs, dtype=torch.float64):
        st = lens.structure
        self.lens, self.specs, self.dtype = lens, specs, dtype
        self.mask, self.mask_G = st.mask_torch.clone(), st.mask_G_torch.clone()
        self.stop = torch.as_tensor(np.asarray(st.stop_idx)).long()
        self.B, self.K = self.mask.shape
        self.last = self.mask.sum(dim=1) - 1
        leaf = lambda a: a.detach().to(dtype).clone().requires_grad_(True)                       # noqa: E731
        self.c, self.t, self.nd = leaf(lens.c), leaf(lens.t), leaf(lens.nd)
        # (the Lens pads v with NaN; a finite filler keeps 0 * NaN out of the backward, the rows are air either way)
        self.v = leaf(torch.where(self.mask_G, lens.v.detach(), torch.ones_like(lens.v.detach())))
        self.kappa = self.poly = None
        if getattr(lens, "kappa", None) is not None:
            self.kappa, self.poly = leaf(lens.kappa), leaf(lens.poly)
        con = lambda a: a.detach().to(dtype)                                                     # noqa: E731
        self.epd, self.hfov = con(specs.epd), con(specs.hfov)
        self.vig = tuple(con(a) for a in (specs.vig_up, specs.vig_down, specs.vig_x))

    def leaves(self):
        return {n: getattr(self, n) for n in LEAVES if getattr(self, n) is not None}

    def flat(self, name, g):
        """A padded gradient as the flat vector of the Lens' leaf: real rows (c, t, kappa, poly) or glass rows (nd, v)."""
        return g[self.mask_G if name in ("nd", "v") else self.mask]

    def tensor(self, values):
        return torch.as_tensor(np.asarray(values, dtype=np.float64)).to(self.dtype)

    # ---- pieces --------------------------------------------------------------------------------------------------
    def indices(self, wavelengths):
        """n [B,K,W]: two-term dispersion through nd and the Abbe number, air rows 1."""
        lam = self.tensor(wavelengths)
        b = (self.nd - 1) / (self.v * (LINES["F"] ** -2 - LINES["C"] ** -2))
        a = self.nd - b / LINES["d"] ** 2
        n = a[..., None] + b[..., None] / lam ** 2
        return torch.where(self.mask_G[..., None], n, torch.ones_like(n))

    @staticmethod
    def mu_of(n):
        """n_{k-1} / n_k with air in front, [B,W,K]."""
        prev = torch.cat((torch.ones_like(n[:, :1]), n[:, :-1]), dim=1)
        return (prev / n).transpose(1, 2)

    @staticmethod
    def chain(c, t, n_d):
        """(A, B, C, D) [B] of M_{K-1} ... M_0, rows multiplied on from left to right: refraction at c from n_{k-1} to n_k,
        then the gap t.  n_d [B,K] is the index behind each row; air in front."""
        B, K = c.shape
        n = torch.cat((torch.ones_like(n_d[:, :1]), n_d), dim=1)
        one, zero = torch.ones(B, dtype=c.dtype), torch.zeros(B, dtype=c.dtype)
        a, b, cc, d = one, zero, zero, one
        for k in range(K):
            r = n[:, k] / n[:, k + 1]
            P = c[:, k] * (r - 1)
            m00, m01, m10, m11 = 1 + P * t[:, k], r * t[:, k], P, r
            a, b, cc, d = m00 * a + m01 * cc, m00 * b + m01 * d, m10 * a + m11 * cc, m10 * b + m11 * d
        return a, b, cc, d

    def n_d(self):
        return torch.where(self.mask_G, self.nd, torch.ones_like(self.nd))

    def front(self):
        """The rows in front of each lens' own stop, padded to the longest front with identity rows: dict(c, t, n_d, mask,
        kappa, poly) [B,Kf]."""
        Kf = int(self.stop.max())
        before = torch.arange(Kf)[None, :] < self.stop[:, None]
        cut = lambda a, fill: torch.where(before.reshape(before.shape + (1,) * (a.dim() - 2)), a[:, :Kf],    # noqa: E731
                                          torch.full_like(a[:, :Kf], fill))
        out = dict(c=cut(self.c, 0.0), t=cut(self.t, 0.0), n_d=cut(self.n_d(), 1.0), mask=self.mask[:, :Kf] & before,
                   mask_G=self.mask_G[:, :Kf] & before, before=before, kappa=None, poly=None)
        if self.kappa is not None:
            out.update(kappa=cut(self.kappa, 0.0), poly=cut(self.poly, 0.0))
        return out

    def full(self):
        return dict(c=self.c, t=self.t, n_d=self.n_d(), mask=self.mask, kappa=self.kappa, poly=self.poly)

    def pupil_z(self):
        """Paraxial entrance-pupil position [B]: B / A of the front's chain, 0 for a stop at row 0."""
        f = self.front()
        if f["c"].shape[1] == 0:
            return torch.zeros(self.B, dtype=self.dtype)
        a, b, _, _ = self.chain(f["c"], f["t"], f["n_d"])
        return b / a

    def first_order(self, wrong=None):
        """(EFL, BFL) [B] from the product of all rows with the last gap zeroed."""
        t = self.t
        if wrong != "last-gap-in":
            t = t * (1 - torch.nn.functional.one_hot(self.last, self.K).to(self.dtype))
        a, _, cc, _ = self.chain(self.c, t, self.n_d())
        return -1 / cc, -a / cc

    def sines(self, fields):
        """cy [B,F]: the correctly rounded fp32 sine of the fp32 angle hfov * field."""
        ang = self.specs.hfov.detach().float()[:, None] * torch.tensor(list(fields), dtype=torch.float32)[None, :]
        return torch.sin(ang.double()).float().to(self.dtype)

    def vignette(self, fields, x, y, vig):
        """Relative pupil points x, y [P] per field: [B,F,P,1] each, squeezed by the linear vignetting function if `vig`."""
        F = len(fields)
        x = self.tensor(x).reshape(1, 1, -1, 1).expand(self.B, F, -1, 1)
        y = self.tensor(y).reshape(1, 1, -1, 1).expand(self.B, F, -1, 1)
        if not vig:
            return x, y
        f = self.tensor(list(fields))[None, :]
        up, down, vx = (linear_vig(f, v)[..., None, None] for v in self.vig)
        return x * (1 - vx), y * (1 - (up + down) / 2) + (down - up) / 2

    def aim_map(self, fields, wavelengths, n_iter, vig, rs=None):
        """(x_scale, y_scale, y_offset) [B,F,1,W] of n_iter aiming steps, detached and rounded to fp32 once; None when
        nothing is aimed (n_iter = 0, or every stop at row 0)."""
        if n_iter == 0 or bool((self.stop == 0).all()):
            return None
        with torch.no_grad():
            inp = AR.inputs(self.lens, self.specs, list(fields), list(wavelengths), z=self.pupil_z().detach())
            tee_ref = None
            if vig:
                xv, yv = self.vignette(fields, [0.0, 0.0, 1.0], [-1.0, 1.0, 0.0], True)
                tee_ref = torch.stack((yv[:, :, 0, 0], yv[:, :, 1, 0], xv[:, :, 2, 0]), dim=-1)
            m = AR.aim(inp, n_iter, tee_ref, None if rs is None else rs.detach())
        return tuple(a.float().to(self.dtype)[:, :, None, :] for a in m)

    def trace(self, rows, x, y, cy, mu):
        """x, y [B,F,P,W] relative pupil points (aimed already) -> image plane of `rows`: the oracle's six outputs."""
        B, K = rows["c"].shape
        dt = self.dtype
        z = self.pupil_z() if self._z is None else self._z
        half = (self.epd / 2).reshape(B, 1, 1, 1)

        def go(sl, kw):
            nb = rows["c"][sl].shape[0]
            return trace_skew_general(x[sl] * half[sl], y[sl] * half[sl], z[sl].reshape(nb, 1, 1, 1), torch.zeros((), dtype=dt),
                                      cy[sl], rows["c"][sl].reshape(nb, 1, 1, 1, K), rows["t"][sl].reshape(nb, 1, 1, 1, K),
                                      mu[sl].reshape(nb, 1, 1, mu.shape[1], K), rows["mask"][sl].reshape(nb, 1, 1, 1, K),
                                      allow_backward_rays=True, ieee_sqrt=(dt == torch.float32), **kw)[:6]
        if rows["kappa"] is None:
            return go(slice(None), {})
        kind = (rows["kappa"].detach() != 0) | (rows["poly"].detach() != 0).any(dim=-1)
        res = [go(slice(b, b + 1), dict(kappa=rows["kappa"][b], poly=rows["poly"][b], kind=[int(k) for k in kind[b]]))
               for b in range(B)]
        return tuple(torch.cat([r[i] for r in res], dim=0) for i in range(6))

    _z = None


def _with_z(S, wrong):
    """Fix the pupil position of one evaluation (attached, or detached for the wrong variant)."""
    z = S.pupil_z()
    S._z = z.detach() if wrong == "z-detached" else z


def distortion(S, fields, wrong=None):
    """(d [B,F], ok [B,F]) of the chief ray on the d line."""
    assert wrong is None or wrong in WRONG
    _with_z(S, wrong)
    try:
        B, F = S.B, len(fields)
        mu = S.mu_of(S.indices([LINES["F" if wrong == "f-line" else "d"]]))
        zero = torch.zeros(B, F, 1, 1, dtype=S.dtype)
        _, y, _, cy, ok, _ = S.trace(S.full(), zero, zero, S.sines(fields).reshape(B, F, 1, 1), mu)
        y, cy = y.reshape(B, F), cy.reshape(B, F)
        efl, bfl = S.first_order(wrong)
        ang = S.tensor(list(fields))[None, :] * S.hfov[:, None]
        ideal = (torch.sin(ang) if wrong == "sin-for-tan" else torch.tan(ang)) * efl[:, None]
        rows = torch.arange(B)
        last = S.last.roll(-1) if wrong == "neighbour-last" else S.last
        defocus = S.t[rows, last] - bfl
        if wrong == "no-defocus":
            defocus = torch.zeros_like(defocus)
        ref_y = ideal + defocus[:, None] * cy / torch.sqrt(1 - cy * cy)
        return (y - ref_y) / ref_y, ok.reshape(B, F)
    finally:
        S._z = None


def relative_illumination(S, fields, wavelengths=("d",), n_iter=1, vig=False, wrong=None):
    """(ri [B,F,W], valid [B,F,W], ok [B,F,3,W]); rays in the order upper, lower, sagittal."""
    assert wrong is None or wrong in WRONG
    assert fields[0] == 0.0
    _with_z(S, wrong)
    try:
        B, F = S.B, len(fields)
        lam = [LINES.get(w, w) for w in wavelengths]
        if wrong == "f-line":
            lam = [LINES["F"] if w == LINES["d"] else w for w in lam]
        W = len(lam)
        ys = [-1.0, 1.0, 0.0] if wrong == "swap-upper-lower" else [1.0, -1.0, 0.0]
        x, y = S.vignette(fields, [0.0, 0.0, 1.0], ys, vig)
        m = S.aim_map(fields, lam, n_iter, vig)
        if m is not None:
            x, y = torch.clamp(x * m[0], -2, 2), torch.clamp(y * m[1] + m[2], -2, 2)
        x, y = x.expand(B, F, 3, W), y.expand(B, F, 3, W)
        _, _, cx, cy, ok, _ = S.trace(S.full(), x, y, S.sines(fields).reshape(B, F, 1, 1), S.mu_of(S.indices(lam)))
        if wrong == "per-wavelength-axis":
            axis = torch.clamp(2 * cy[:, 0, 0, :] ** 2, min=1e-6)[:, None, :]
        else:
            axis = torch.clamp(2 * cy[:, 0, 0, 0] ** 2, min=1e-6)[:, None, None]
        sag = cy[:, :, 2, :] if wrong == "sagittal-cy" else cx[:, :, 2, :]
        ri = (cy[:, :, 0, :] - cy[:, :, 1, :]) * sag / axis
        valid = ok.all(dim=2)
        valid = valid & valid[:, :1, :]
        return torch.where(valid, ri, torch.ones_like(ri)), valid, ok
    finally:
        S._z = None


def ray_aiming_error(S, fields, n_iter=1, vig=False, mode="real", wrong=None):
    """(e [B,F,2,1], ok [B,F,2,1]) of the lower and the upper meridional ray at the stop, d line; (0, None) when every
    stop is row 0."""
    assert wrong is None or wrong in WRONG
    assert mode in ("real", "paraxial")
    if bool((S.stop == 0).all()):
        return 0, None
    _with_z(S, wrong)
    try:
        B, F = S.B, len(fields)
        f = S.front()
        Kf = f["c"].shape[1]
        mu_d = S.mu_of(f["n_d"][..., None])
        if mode == "paraxial":
            rs = S.chain(f["c"], f["t"], f["n_d"])[0] * S.epd / 2
        else:
            zero = torch.zeros(B, 1, 1, 1, dtype=S.dtype)
            rs = S.trace(f, zero, zero + 1, torch.zeros(B, 1, 1, 1, dtype=S.dtype), mu_d)[1].reshape(B)
        x, y0 = S.vignette(fields, [0.0, 0.0], [-1.0, 1.0], False)
        _, yv = S.vignette(fields, [0.0, 0.0], [-1.0, 1.0], vig)
        m = S.aim_map(fields, [LINES["d"]], n_iter, vig, rs if mode == "paraxial" else None)
        ya = yv if m is None else torch.clamp(yv * m[1] + m[2], -2, 2)
        mu = mu_d
        if wrong == "f-line":
            n_f = S.indices([LINES["F"]])[:, :Kf]
            mu = S.mu_of(torch.where(f["before"][..., None], n_f, torch.ones_like(n_f)))
        _, ys, _, _, ok, _ = S.trace(f, x, ya, S.sines(fields).reshape(B, F, 1, 1), mu)
        return ys / rs.reshape(B, 1, 1, 1) - (y0 if wrong == "unvignetted-height" else yv), ok
    finally:
        S._z = None


def weights(shape, seed):
    """Fixed weights of order 1 (0.5 .. 1.5), so that no component of a metric cancels in the loss sum(w metric)."""
    return torch.from_numpy(np.random.default_rng(seed).uniform(0.5, 1.5, size=tuple(shape)))


def leaf_gradients(S, value, w):
    """{leaf: flat gradient of sum(w value)} as fp64 numpy, in the layout of the Lens' flat leaves."""
    lv = S.leaves()
    gs = torch.autograd.grad((w.to(S.dtype) * value).sum(), list(lv.values()), allow_unused=True)
    return {n: S.flat(n, torch.zeros_like(lv[n]) if g is None else g).detach().double().numpy()
            for (n, _), g in zip(lv.items(), gs)}
