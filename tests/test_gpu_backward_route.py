"""
The C ABI of tl_trace_fwd / tl_trace_bwd / tl_trace_bwd_from_outputs held to the words of include/tl_trace.h: which kernels a
backward call enqueues (tl_bwd_route), witnessed on the device, and the nullable members of the three pointer blocks.

The witness.  Each cell computes the gradients twice on the same forward outputs and seeds: with tl_trace_bwd_from_outputs and
with tl_trace_bwd.  Where the header says the checkpoint kernel does all the work (the call is handed to tl_trace_bwd: the
penalty term outside 3..20 rows, below 256 pupil points or without stored aspheric hits; a lens with more aspheric rows than hit
slots, on the device; an ill-conditioned fan without per-ray flags) the two results are EQUAL IN EVERY BIT.  Where it says a
walk-back kernel ran, at least one element of the concatenated gradient DIFFERS: the walk-back rebuilds every ray from the image
plane, so its sums carry other roundings.  (That is a property of the inputs, not a tolerance: a cell that came out equal where a
walk-back did the work would get a larger pupil, and none needed one.)  In both cases each gradient stays inside test_gpu_kernel_matrix._gate of the fp64 oracle.

The header names one more way for the checkpoint kernel to take a whole launch: the walk-back met a non-finite adjoint and
flagged the word at the end of the workspace.  The test clears that word before each tl_trace_bwd_from_outputs call and reads it
afterwards, so the third case is seen, not guessed: a flagged launch must have tl_trace_bwd's bits, an unflagged one must differ.
An all-spherical lens and every unrolled walk-back of a lens whose aspheric rows fit the hit slots must not flag it at all.
Measured on the MI355X: the ROLLED ASPHERIC walk-back (trace_bwd_inv_kernel<true>, Newton on the reversed ray) flags it in
every cell of these fans -- 31 of 31, strict and fast, 2 to 21 rows, with and without stored hits -- so on them that kernel
never does the work (`flagged` in the ROUTE line; the gradients are the checkpoint kernel's, and right).  The cause is the DEAD
rays every _fan holds: the same fans with the pupil points of the dead rays replaced by a live point are walked back, unflagged
(test_rolled_aspheric_walk_back_does_the_work_on_a_fan_without_dead_rays: the same cells on such a fan, so that the kernel is
held to the oracle after all).  Read in the kernel, not proven: at row 0 it forms the aspheric row's adjoint from the ray's real
launch point, and a dead ray of these fans is one that missed row 0 -- a NaN times a zero seed.  That is a finding about device
code, which this change does not touch: ADVICE.md has it.

Cells: kernel_matrix._fan(S, variant, P), S in {2, 3, 20, 21} (both sides of the unrolled range) x P in {255, 256} (both sides
of the smallest pupil the unrolled kernels take) x {rms, rms + lam sumQ} x {spherical; aspheric with hits stored; aspheric with
asph_hits NULL; aspheric with asph_hit_slots 0 -- and asph_hits NULL, check_problem refuses the pointer next to 0 slots; 'asph5'
with 4 slots, which needs 15 rows: S = 20, 21}, strict; fast at S = 20.  The forward always leaves the per-ray conditioning
flags, as the host chains have it: a fan with a flagged ray is then split, not handed over.  Fixture G5 (flagged and dead rays)
with its own pupil and the 205-point slice: flags with moments (split: differ), no flags with moments (checkpoint: equal), no
flags and no moments (walked back anyway: differ, every parameter at the looser launch-condition gate), flags without moments
(refused).

One line per cell:  ROUTE <cell>: <route> <equal|differ> worst e64/gate <x>.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_kernel_matrix as km
from test_gpu_conditioning import _g5

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
SLOTS = 4
ROWS_ROUTE = (2, 3, 20, 21)
PUPILS_ROUTE = (255, 256)
# (name of the hit variant, asph_hits kept, asph_hit_slots) as tl_trace_bwd_from_outputs sees them; the forward stored the hits
HIT_VARIANTS = {"sph": (("sph", True, 0),),
                "asph": (("hits", True, SLOTS), ("hits_null", False, SLOTS), ("slots0", False, 0)),
                "asph5": (("hits", True, SLOTS),)}
LENS_CELLS = ([(S, v, P, "strict") for S in ROWS_ROUTE for P in PUPILS_ROUTE for v in ("sph", "asph")]
              + [(S, "asph5", P, "strict") for S in (20, 21) for P in PUPILS_ROUTE]
              + [(20, v, P, "fast") for P in PUPILS_ROUTE for v in ("sph", "asph", "asph5")])
G5_PUPILS = {"fixture": None, "slice205": slice(0, 1024, 5)}


@pytest.fixture(scope="module")
def lib():
    from torchoptics_amd import _lib
    return _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Launch:
    """The device tensors of one lens (`a`: a kernel_matrix._fan dict) behind a tl_problem, and the three calls on them."""

    def __init__(self, a, pen, mode, n_index=False):
        from torchoptics_amd import _lib, ops
        self._lib, self.lib = _lib, _lib.lib()
        d = lambda t: t.to(DEV).contiguous()                                             # noqa: E731
        F, P, W = a["cy"].shape[1], a["x"].shape[2], a["mu"].shape[3]
        S = a["c"].shape[-1]
        self.F, self.P, self.W, self.S, self.pen = F, P, W, S, pen
        self.asph = bool(a.get("rows"))
        x_e, y_e = d(a["x"].expand(1, F, P, W)), d(a["y"].expand(1, F, P, W))
        keep = [x_e, y_e, d(a["z"].reshape(1)), d(a["cx"].reshape(1, -1)), d(a["cy"].reshape(1, -1)), d(a["c"].reshape(1, S)),
                d(a["t"].reshape(1, S)), d(a["mu"].reshape(1, W, S)), d(a["mask"].reshape(1, S).to(torch.uint8))]
        kap = pol = kind = hits = nidx = None
        if self.asph:
            kap, pol = d(a["kappa"].reshape(1, S)), d(a["poly"].reshape(1, S, 4))
            kind = d(torch.tensor(a["kind"], dtype=torch.uint8).reshape(1, S))
            hits = torch.empty((min(SLOTS, S), 2, 1, F, W, P), dtype=torch.float32, device=DEV)
        if n_index:
            n = [torch.ones(1, W, dtype=torch.float64)]
            for k in range(S):
                n.append(n[-1] / a["mu"].reshape(1, W, S)[..., k].double())
            nidx = d(torch.stack(n, dim=-1).float())                                       # [1,W,S+1]
        self.cond = torch.empty((1, F, W, P), dtype=torch.uint8, device=DEV)
        self.hits = hits
        self.keep = keep + [kap, pol, kind, nidx]             # (tl_problem holds raw pointers: these outlive every call)
        self.prob = ops._problem(*keep, True, mode, kap, pol, kind, nidx, pen, hits, False, self.cond)
        self.ws = torch.zeros(self.lib.tl_workspace_bytes(C.byref(self.prob)), dtype=torch.uint8, device=DEV)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def variant(self, **members):
        """A copy of the problem with some members replaced (asph_hits, asph_hit_slots, cond_flags, B, aggregate, n_index)."""
        q = self._lib.tl_problem.from_buffer_copy(self.prob)
        for k, v in members.items():
            setattr(q, k, v)
        return q

    def new_rays(self, members=None, prob=None):
        """Sentinel-filled buffers for the named members of tl_rays (default: all this problem can write)."""
        pen = self.pen if prob is None else bool(prob.aggregate)
        F, P, W, S = self.F, self.P, self.W, self.S
        shapes = dict(x=((1, F, W, P), torch.float32), y=((1, F, W, P), torch.float32), cx=((1, F, W, P), torch.float32),
                      cy=((1, F, W, P), torch.float32), ok=((1, F, W, P), torch.uint8), back=((1, F, W, P), torch.uint8),
                      opd=((1, F, W, P), torch.float32), stacks=((3, S, 1, F, W, P), torch.float32),
                      moments=((F, self._lib.TL_NMOM), torch.float64))
        if members is None:
            members = [m for m in shapes if m != ("opd" if pen else "stacks") and (m != "opd" or self.keep[-1] is not None)]
        out = {}
        for m in members:
            shape, dt = shapes[m]
            out[m] = torch.full(shape, 77, dtype=dt, device=DEV) if dt == torch.uint8 else torch.full(shape, -7.25, dtype=dt, device=DEV)
        return out

    def fwd(self, rays, prob=None):
        p = self.prob if prob is None else prob
        return self.lib.tl_trace_fwd(C.byref(p), self._lib.rays(**rays), self._lib.ptr(self.ws), self.ws.numel(), self.st)

    def g_moments(self, mom, lam):
        """d(rms + lam sumQ / S) / d moments: tl_spot_rms' derivative, plus the penalty's uniform seed in entry 8."""
        rms = torch.empty((), dtype=torch.float32, device=DEV)
        dm = torch.empty_like(mom)
        rc = self.lib.tl_spot_rms(0, 1, self.F, float(self.P * self.W), self._lib.ptr(mom), self._lib.ptr(rms), self._lib.ptr(dm),
                                  self.st)
        assert rc == 0, self.lib.tl_last_error()
        if self.pen:
            dm[:, 8] += lam / self.S
        return dm

    def bwd(self, how, gmom, rays=None, prob=None, moments=True, ok=True, per_ray=()):
        """tl_trace_bwd ('bwd') or tl_trace_bwd_from_outputs ('from_outputs') into fresh sentinel-filled gradient buffers.
        Returns (rc, {name: tensor})."""
        p = self.prob if prob is None else prob
        F, P, W, S = self.F, self.P, self.W, self.S
        sizes = dict(g_c=(1, S), g_t=(1, S), g_mu=(1, W, S), g_z=(1,), g_cx=(1, F), g_cy=(1, F))
        if self.asph:
            sizes.update(g_kappa=(1, S), g_poly=(1, S, 4))
        for m in per_ray:
            sizes[m] = (1, F, W, P)
        g = {m: torch.full(s, -7.25, dtype=torch.float32, device=DEV) for m, s in sizes.items()}
        seeds, grads = self._lib.seeds(g_moments=gmom), self._lib.grads(**g)
        if how == "bwd":
            rc = self.lib.tl_trace_bwd(C.byref(p), seeds, grads, self._lib.ptr(self.ws), self.ws.numel(), self.st)
        else:
            self.ws[-64:-60].zero_()              # the walk-back's flag word (64 bytes before the end of tl_workspace_bytes)
            f = self._lib.rays(x=rays["x"], y=rays["y"], cx=rays["cx"], cy=rays["cy"], ok=rays["ok"] if ok else None,
                               moments=rays["moments"] if moments else None)
            rc = self.lib.tl_trace_bwd_from_outputs(C.byref(p), seeds, f, grads, self._lib.ptr(self.ws), self.ws.numel(), self.st)
        return rc, g

    def flagged(self):
        """Whether the walk-back of the last tl_trace_bwd_from_outputs call met a non-finite adjoint: it then wrote the call's
        token (never 0) into the word that `bwd` cleared."""
        return bool(self.ws[-64:-60].view(torch.int32).item() != 0)


_LEAF_OF = dict(z="g_z", cy="g_cy", c="g_c", t="g_t", mu="g_mu", kappa="g_kappa", poly="g_poly")


def _as_leaves(g, names):
    """The C ABI's gradient arrays under the oracle's leaf names, as CPU doubles (rel_l2 compares them flattened: [W,S] is
    the order of mu [1,1,1,W,S], [S,4] of poly)."""
    return {n: g[_LEAF_OF[n]].detach().cpu().double().reshape(-1) for n in names}


def _concat(g):
    return torch.cat([g[m].reshape(-1) for m in sorted(g)])


def _worst_over_gate(got, r32, r64, pen, k, cancel=None, loose=False):
    """max over the parameters of e64 / gate, with e64, noise and the gate exactly as kernel_matrix._grad_errors forms them;
    `loose`: every parameter at the launch-condition gate (that of z and cy)."""
    worst = 0.0
    for n, g in got.items():
        w32, w64 = r32[n], r64[n]
        if n in km._PER_RAY:
            d = (w32 - w64).abs()
            w32, w64 = km._reduce(n, w32, g), km._reduce(n, w64, g)
            e64, noise = km.rel_l2(g.numpy(), w64.numpy()), km.rel_l2(w32.numpy(), w64.numpy())
            if n == "z":
                noise = max(noise, float(km._reduce(n, d, g).norm() / w64.norm()))
        else:
            e64, noise = km.rel_l2(g.numpy(), w64.numpy()), km.rel_l2(w32.numpy(), w64.numpy())
        gate = km._gate("z" if loose else n, pen, noise, k, 1.0 if cancel is None else cancel[n])
        worst = max(worst, e64 / gate)
    return worst


def _expected(S, P, pen, lens, hit_variant, lib, prob):
    """(route name, 'equal' | 'differ') from the header's words, and tl_bwd_route's own answer checked against them."""
    from torchoptics_amd import ops
    hits_ok = lens == "sph" or hit_variant == "hits"
    if 3 <= S <= 20 and P >= 256 and hits_ok:
        route = "walk_unrolled"
    else:
        route = "checkpoint" if pen else "walk_rolled"
    assert ops.BACKWARD_ROUTES[lib.tl_bwd_route(C.byref(prob))] == route
    # more aspheric rows than hit slots: the unrolled walk-back hands the lens to the checkpoint kernel on the device
    handed = route == "checkpoint" or (route == "walk_unrolled" and lens == "asph5")
    return route, "equal" if handed else "differ"


@pytest.mark.parametrize("S,lens,P,mode", LENS_CELLS, ids=[f"S{s}-{v}-P{p}-{m}" for s, v, p, m in LENS_CELLS])
def test_route_is_witnessed_by_the_bits_of_the_two_backward_calls(lib, S, lens, P, mode):
    r = km._oracle(S, lens, P)
    a, names = r["args"], r["names"]
    k = 10.0 if mode == "fast" else 1.0
    for pen in (False, True):
        lam = r["lam"] if pen else 0.0
        L = _Launch(a, pen, mode)
        rays = L.new_rays()
        assert L.fwd(rays) == 0, lib.tl_last_error()
        gmom = L.g_moments(rays["moments"], lam)
        ref32, ref64 = km._ref_grad(r["f32"], pen, lam), km._ref_grad(r["f64"], pen, lam)
        cancel = km._cancel(km._parts(r["f64"], lam)) if pen else None
        for hv, keep_hits, slots in HIT_VARIANTS[lens]:
            prob = L.prob if lens == "sph" else L.variant(asph_hits=L.prob.asph_hits if keep_hits else None, asph_hit_slots=slots)
            route, want = _expected(S, P, pen, lens, hv, lib, prob)
            tag = f"S={S} P={P} {lens}/{hv} {'pen' if pen else 'rms'} {mode}"
            rc, g_out = L.bwd("from_outputs", gmom, rays, prob)
            assert rc == 0, (tag, lib.tl_last_error())
            rc, g_bwd = L.bwd("bwd", gmom, prob=prob)
            assert rc == 0, (tag, lib.tl_last_error())
            torch.cuda.synchronize()
            same, flagged = _same_bits(_concat(g_out), _concat(g_bwd)), L.flagged()
            worst = 0.0
            for which, g in (("from_outputs", g_out), ("bwd", g_bwd)):
                got = _as_leaves(g, names)
                worst = max(worst, _worst_over_gate(got, ref32, ref64, pen, k, cancel))
                km._grad_errors(f"{tag} {which}", got, ref32, ref64, pen, k, a["rows"], S, cancel)
            print(f"ROUTE {tag}: {route} {'equal' if same else 'differ'}{' flagged' if flagged else ''} worst e64/gate {worst:.2f}")
            if want == "equal":
                assert same, f"{tag}: route {route}, the checkpoint kernel does all the work: the two calls' bits should be equal"
            else:
                # a walk-back that must do the work: every all-spherical lens, every unrolled kernel
                assert not (flagged and (lens == "sph" or route == "walk_unrolled")), f"{tag}: the walk-back met a non-finite adjoint"
                assert same is flagged, f"{tag}: route {route}, flag word {'set' if flagged else 'clear'}, bits {'equal' if same else 'differ'}"


def _rolled_variants(S, lens, P):
    """The hit variants of an aspheric cell that the rolled walk-back takes without the penalty term."""
    return [v for v in HIT_VARIANTS[lens] if not (3 <= S <= 20 and P >= 256 and v[0] == "hits")]


ROLLED_CELLS = [c for c in LENS_CELLS if c[1] != "sph" and _rolled_variants(c[0], c[1], c[2])]
_ALIVE = {}


def _alive_case(S, lens, P):
    """kernel_matrix._fan(S, lens, P) with every pupil point that holds a dead ray (any field or wavelength, fp32 or fp64
    oracle) replaced by the first point that holds none, and the oracle's fp32 / fp64 gradients of rms on that fan."""
    key = (S, lens, P)
    if key in _ALIVE:
        return _ALIVE[key]
    from oracle import trace_oracle as orc
    r = km._oracle(S, lens, P)
    a = dict(r["args"])
    ok = r["f32"]["fwd"][4] & r["f64"]["fwd"][4]                                    # [1,F,P,W]
    dead = ~ok.all(dim=3).all(dim=1).reshape(-1)
    assert dead.any() and not dead.all()
    j = int((~dead).nonzero()[0])
    a["x"], a["y"] = a["x"].clone(), a["y"].clone()
    a["x"][:, :, dead], a["y"][:, :, dead] = a["x"][:, :, j:j + 1].clone(), a["y"][:, :, j:j + 1].clone()
    res = dict(args=a, names=r["names"])
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        lv = {n: (a[n].to(dt).expand(a["x"].shape) if n in km._PER_RAY else a[n].to(dt)).clone().requires_grad_(True)
              for n in r["names"]}
        o = orc.trace_skew_general(a["x"].to(dt), a["y"].to(dt), lv["z"], a["cx"].to(dt), lv["cy"], lv["c"], lv["t"], lv["mu"],
                                   a["mask"], ieee_sqrt=(dt == torch.float32), kappa=lv["kappa"], poly=lv["poly"], kind=a["kind"])
        assert o[4].all()
        g = torch.autograd.grad(orc.compute_rms2d(o[0], o[1], o[4]), [lv[n] for n in r["names"]])
        res[tag] = {n: v.double() for n, v in zip(r["names"], g)}
    _ALIVE[key] = res
    return res


@pytest.mark.parametrize("S,lens,P,mode", ROLLED_CELLS, ids=[f"S{s}-{v}-P{p}-{m}" for s, v, p, m in ROLLED_CELLS])
def test_rolled_aspheric_walk_back_does_the_work_on_a_fan_without_dead_rays(lib, S, lens, P, mode):
    """The cells of the test above that the rolled aspheric walk-back takes (rms; the penalty term is handed over), on the same
    fans without their dead rays: the flag word stays clear, the bits differ from tl_trace_bwd's, both within the gate."""
    r = _alive_case(S, lens, P)
    a, names = r["args"], r["names"]
    k = 10.0 if mode == "fast" else 1.0
    L = _Launch(a, False, mode)
    rays = L.new_rays()
    assert L.fwd(rays) == 0, lib.tl_last_error()
    assert bool(rays["ok"].all())
    gmom = L.g_moments(rays["moments"], 0.0)
    for hv, keep_hits, slots in _rolled_variants(S, lens, P):
        prob = L.variant(asph_hits=L.prob.asph_hits if keep_hits else None, asph_hit_slots=slots)
        route, _ = _expected(S, P, False, lens, hv, lib, prob)
        assert route == "walk_rolled"
        tag = f"S={S} P={P} {lens}/{hv} rms {mode}, no dead rays"
        rc, g_out = L.bwd("from_outputs", gmom, rays, prob)
        assert rc == 0, (tag, lib.tl_last_error())
        rc, g_bwd = L.bwd("bwd", gmom, prob=prob)
        assert rc == 0, (tag, lib.tl_last_error())
        torch.cuda.synchronize()
        same, flagged = _same_bits(_concat(g_out), _concat(g_bwd)), L.flagged()
        worst = 0.0
        for which, g in (("from_outputs", g_out), ("bwd", g_bwd)):
            got = _as_leaves(g, names)
            worst = max(worst, _worst_over_gate(got, r["f32"], r["f64"], False, k))
            km._grad_errors(f"{tag} {which}", got, r["f32"], r["f64"], False, k, a["rows"], S)
        print(f"ROUTE {tag}: {route} {'equal' if same else 'differ'}{' flagged' if flagged else ''} worst e64/gate {worst:.2f}")
        assert not flagged and not same, f"{tag}: flag word {'set' if flagged else 'clear'}, bits {'equal' if same else 'differ'}"


_G5_ORACLE = {}


def _g5_case(pupil):
    """Fixture G5 with the given pupil as a _fan-like dict, and the oracle's fp32 / fp64 gradients of rms in the format of
    kernel_matrix._oracle (z and cy per ray)."""
    if pupil in _G5_ORACLE:
        return _G5_ORACLE[pupil]
    from oracle import trace_oracle as orc
    ins, mask = _g5(G5_PUPILS[pupil])
    F, P, W = ins[4].shape[1], ins[0].shape[2], ins[7].shape[3]
    a = dict(zip(("x", "y", "z", "cx", "cy", "c", "t", "mu"), ins), mask=mask, rows=[])
    a["x"], a["y"] = a["x"].expand(1, F, P, W), a["y"].expand(1, F, P, W)
    res = dict(args=a, names=km._LEAVES)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        lv = {n: (a[n].to(dt).expand(1, F, P, W) if n in km._PER_RAY else a[n].to(dt)).clone().requires_grad_(True)
              for n in km._LEAVES}
        o = orc.trace_skew_general(a["x"].to(dt), a["y"].to(dt), lv["z"], a["cx"].to(dt), lv["cy"], lv["c"], lv["t"], lv["mu"],
                                   mask, ieee_sqrt=(dt == torch.float32))
        g = torch.autograd.grad(orc.compute_rms2d(o[0], o[1], o[4]), [lv[n] for n in km._LEAVES])
        res[tag] = dict(g_rms={n: v.double() for n, v in zip(km._LEAVES, g)})
    _G5_ORACLE[pupil] = res
    return res


@pytest.mark.parametrize("pupil", tuple(G5_PUPILS))
def test_flags_and_moments_decide_who_takes_the_ill_conditioned_rays(lib, pupil):
    r = _g5_case(pupil)
    a = r["args"]
    L = _Launch(a, False, "strict")
    rays = L.new_rays()
    assert L.fwd(rays) == 0, lib.tl_last_error()
    n_ill, n_ok = int(rays["moments"][:, 9].sum().item()), int(rays["ok"].sum().item())
    assert 0 < n_ill < n_ok < rays["ok"].numel(), (n_ill, n_ok)         # flagged, unflagged and dead rays in one launch
    assert int((L.cond == 2).sum().item()) == n_ill
    gmom = L.g_moments(rays["moments"], 0.0)
    no_flags = L.variant(cond_flags=None)
    rc, g_bwd = L.bwd("bwd", gmom, prob=no_flags)
    assert rc == 0, lib.tl_last_error()
    ref32, ref64 = r["f32"]["g_rms"], r["f64"]["g_rms"]
    cells = (("flags, moments", L.prob, True, "differ", False), ("no flags, moments", no_flags, True, "equal", False),
             ("no flags, no moments", no_flags, False, "differ", True))
    for name, prob, with_mom, want, loose in cells:
        rc, g = L.bwd("from_outputs", gmom, rays, prob, moments=with_mom)
        assert rc == 0, (name, lib.tl_last_error())
        torch.cuda.synchronize()
        same = _same_bits(_concat(g), _concat(g_bwd))
        assert not L.flagged(), f"G5 {pupil} {name}: the walk-back met a non-finite adjoint"
        got = _as_leaves(g, km._LEAVES)
        worst = max(_worst_over_gate(got, ref32, ref64, False, 1.0, loose=loose),
                    _worst_over_gate(_as_leaves(g_bwd, km._LEAVES), ref32, ref64, False, 1.0))
        from torchoptics_amd import ops
        route = ops.BACKWARD_ROUTES[lib.tl_bwd_route(C.byref(prob))]
        print(f"ROUTE G5 {pupil} P={L.P} {name} ({n_ill} of {n_ok} live rays flagged): {route} "
              f"{'equal' if same else 'differ'} worst e64/gate {worst:.2f}")
        assert same is (want == "equal"), f"G5 {pupil} {name}: the two calls' bits should {want}"
        assert all(torch.isfinite(v).all() for v in got.values())
        assert worst <= 1.0, f"G5 {pupil} {name}: worst e64 / gate {worst:.2f}"
    # flags without moments: the checkpoint kernel would never take the rays flagged 2 -- refused, nothing launched or written
    rc, g = L.bwd("from_outputs", gmom, rays, L.prob, moments=False)
    msg = lib.tl_last_error()
    assert rc == EINVAL and b"cond_flags" in msg and b"moments" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert all(bool((v == -7.25).all()) for v in g.values())


# ------------------------------------------------------------------------------------------------------------------
# the nullable members of the three blocks, on the smallest fans above
# ------------------------------------------------------------------------------------------------------------------

def test_flags_without_moments_are_refused_on_every_route(lib):
    for S, lens, P, pen in ((3, "sph", 256, False), (3, "sph", 255, False), (3, "sph", 256, True), (3, "sph", 255, True),
                            (2, "asph", 256, False)):
        L = _Launch(km._oracle(S, lens, P)["args"], pen, "strict")
        rays = L.new_rays()
        assert L.fwd(rays) == 0, lib.tl_last_error()
        gmom = L.g_moments(rays["moments"], 0.1)
        rc, g = L.bwd("from_outputs", gmom, rays, moments=False)
        msg = lib.tl_last_error()
        assert rc == EINVAL and b"cond_flags" in msg and b"moments" in msg, (S, lens, P, pen, rc, msg)
        torch.cuda.synchronize()
        assert all(bool((v == -7.25).all()) for v in g.values()), "a refused call wrote a gradient"
        rc, _ = L.bwd("from_outputs", gmom, rays, L.variant(cond_flags=None), moments=False)      # no flags: nullable, as before
        assert rc == 0, lib.tl_last_error()


@pytest.mark.parametrize("kind", ("penalty", "opd"))
def test_forward_writes_the_same_bits_whichever_members_are_asked_for(lib, kind):
    """A problem with n_index, hit slots and flags; `penalty`: aggregate (stacks, moment 8; the opd member is refused next to
    it), `opd`: the path length.  Each member of tl_rays alone (moments alone included) and all members but one: every array
    written has the bits of the all-members call, cond_flags and asph_hits are the same bytes every time."""
    a = km._oracle(3, "asph", 256)["args"]
    L = _Launch(a, kind == "penalty", "strict", n_index=True)
    if kind == "penalty":
        rc = L.fwd(L.new_rays(["x", "opd"]))
        assert rc == EINVAL and b"opd" in lib.tl_last_error()

    def call(members):
        L.cond.fill_(77)
        L.hits.fill_(-7.25)
        rays = L.new_rays(members)
        assert L.fwd(rays) == 0, (members, lib.tl_last_error())
        torch.cuda.synchronize()
        return rays, L.cond.clone(), L.hits.clone()
    full, cond, hits = call(None)
    names = list(full)
    assert ("stacks" in names) is (kind == "penalty") and ("opd" in names) is (kind == "opd") and len(names) == 8
    assert int(cond.max().item()) <= 2 and torch.equal(cond != 0, full["ok"] != 0) and not bool((full["ok"] == 77).any())
    assert not bool((hits[:3] == -7.25).all())
    subsets = [[m] for m in names] + [[m for m in names if m != drop] for drop in names]
    for members in subsets:
        rays, cond_s, hits_s = call(members)
        for m in members:
            assert _same_bits(rays[m], full[m]), f"{kind}: member {m} of the call for {members}"
        assert torch.equal(cond_s, cond), f"{kind}: cond_flags after the call for {members}"
        assert _same_bits(hits_s, hits), f"{kind}: asph_hits after the call for {members}"


@pytest.mark.parametrize("pen", (False, True))
def test_zero_lenses_is_read_as_one(lib, pen):
    """tl_problem.B = 0 (a caller of the ABI before the lens batch zero-initialises it): the three calls give the bits of B = 1."""
    r = km._oracle(3, "asph", 256)
    L = _Launch(r["args"], pen, "strict")
    res = {}
    for B in (1, 0):
        prob = L.variant(B=B)
        assert lib.tl_workspace_bytes(C.byref(prob)) == L.ws.numel()
        rays = L.new_rays()
        assert L.fwd(rays, prob) == 0, lib.tl_last_error()
        gmom = L.g_moments(rays["moments"], r["lam"])
        rc1, g1 = L.bwd("from_outputs", gmom, rays, prob)
        rc2, g2 = L.bwd("bwd", gmom, prob=prob)
        assert rc1 == 0 and rc2 == 0, lib.tl_last_error()
        torch.cuda.synchronize()
        res[B] = (rays, L.cond.clone(), L.hits.clone(), g1, g2)
    for m in res[1][0]:
        assert _same_bits(res[0][0][m], res[1][0][m]), m
    assert torch.equal(res[0][1], res[1][1]) and _same_bits(res[0][2], res[1][2])
    for i in (3, 4):
        assert _same_bits(_concat(res[0][i]), _concat(res[1][i])), ("from_outputs", "bwd")[i - 3]


_XY_ORACLE = {}


def _oracle_xy(S, lens, P):
    """d rms / d x_in, d rms / d y_in per ray [1,F,P,W] in fp32 (IEEE sqrt) and fp64."""
    key = (S, lens, P)
    if key not in _XY_ORACLE:
        from oracle import trace_oracle as orc
        a = km._oracle(S, lens, P)["args"]
        out = {}
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            xl, yl = (a[n].to(dt).clone().requires_grad_(True) for n in ("x", "y"))
            o = orc.trace_skew_general(xl, yl, *[a[n].to(dt) for n in ("z", "cx", "cy", "c", "t", "mu")], a["mask"],
                                       ieee_sqrt=(dt == torch.float32))
            gx, gy = torch.autograd.grad(orc.compute_rms2d(o[0], o[1], o[4]), [xl, yl])
            out[tag] = dict(g_x_in=gx.double(), g_y_in=gy.double())
        _XY_ORACLE[key] = out
    return _XY_ORACLE[key]


@pytest.mark.parametrize("S,P", ((3, 256), (2, 255)))
def test_one_per_ray_input_gradient_alone(lib, S, P):
    """tl_trace_bwd asked for g_x_in only, or g_y_in only, beside the required outputs: those keep the bits of the call that
    asks for neither, and the per-ray gradient is the fp64 oracle's within the launch-condition gate of the kernel matrix."""
    a = km._oracle(S, "sph", P)["args"]
    want = _oracle_xy(S, "sph", P)
    L = _Launch(a, False, "strict")
    rays = L.new_rays()
    assert L.fwd(rays) == 0, lib.tl_last_error()
    gmom = L.g_moments(rays["moments"], 0.0)
    rc, base = L.bwd("bwd", gmom)
    assert rc == 0, lib.tl_last_error()
    for member in ("g_x_in", "g_y_in"):
        rc, g = L.bwd("bwd", gmom, per_ray=(member,))
        assert rc == 0, (member, lib.tl_last_error())
        torch.cuda.synchronize()
        per_ray = g.pop(member).cpu().double().permute(0, 1, 3, 2)                  # [1,F,W,P] -> [1,F,P,W]
        assert _same_bits(_concat(g), _concat(base)), f"{member}: the required outputs changed"
        e64 = km.rel_l2(per_ray.numpy(), want["f64"][member].numpy())
        noise = km.rel_l2(want["f32"][member].numpy(), want["f64"][member].numpy())
        gate = km._gate("z", False, noise, 1.0)
        print(f"S={S} P={P} {member} alone: vs fp64 {e64:.2e}, oracle fp32 itself {noise:.2e}, e64/gate {e64 / gate:.2f}")
        assert torch.isfinite(per_ray).all() and e64 <= gate, (member, e64, gate)
        dead = ~rays["ok"].bool().permute(0, 1, 3, 2).cpu()
        assert not per_ray[dead].any(), f"{member}: a dead ray carries a gradient"
