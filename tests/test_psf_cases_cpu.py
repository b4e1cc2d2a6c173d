"""tests/psf_cases.py without a GPU: the Python mirror of the launch plan equals the library's (tl_psf_workspace_bytes is
host-only) and every case lands on the branch its row states; the bounds are SUFFICIENT (a float32 emulation of the kernels'
arithmetic stays within them on every case) and SHARP (eight deliberately wrong float64 evaluations exceed them); the float32
torch definition that tests/test_gpu_psf_fused.py uses agrees with tests/psf_ref.py."""
import numpy as np
import pytest
import torch

import psf_cases as pc
import psf_ref as ref
from test_gpu_psf_fused import _hist_torch
from torchoptics_amd import _lib


# ------------------------------------------------------------------------------------------------------- the plan mirror

def test_every_case_lands_on_the_plan_its_row_states_and_all_eight_instantiations_are_used():
    used = set()
    for name, (G, W, R, ny, nxh, _, _) in pc.CASES.items():
        pl = pc.plan(G, W, R, nxh, ny)
        assert (pl.nb, pl.nbx_fwd, pl.rpl, pl.nbx_bwd, pl.nxp) == pc.EXPECT[name], name
        assert G != W or G == 1, name
        used.add(pl.nxp)
    assert used == {4, 12, 20, 24, 28, 32}
    G, W, R, ny = pc.SWEEP_SHAPE
    sweep = {pc.plan(G, W, R, nxh, ny).nxp for nxh in pc.SWEEP_NXH}
    assert sweep == {4, 8, 12, 16, 20, 24, 28, 32} == used | sweep
    assert any(pc.EXPECT[n][0] > 1 and pc.EXPECT[n][1] > 1 for n in pc.CASES), "no case with nb > 1 over several blocks"
    assert any(pc.EXPECT[n][2] > 1 for n in pc.CASES), "no case with rpl > 1"


def test_the_plan_mirror_gives_the_workspace_size_of_the_library():
    dll = _lib.lib()
    shapes = [(G, W, R, nxh, ny) for (G, W, R, ny, nxh, _, _) in pc.CASES.values()]
    shapes += [pc.SWEEP_SHAPE[:3] + (nxh, pc.SWEEP_SHAPE[3]) for nxh in pc.SWEEP_NXH]
    clamps = [(255, 257, 1088, 2, 2), (255, 257, 64 * 17 + 1, 32, 32), (1, 1, 1 << 26, 11, 21), (3, 3, 1 << 24, 32, 1),
              (1, 1, (1 << 25) + 1, 1, 32)]
    assert {pc.plan(*s).nb for s in clamps} >= {256} and {pc.plan(*s).rpl for s in clamps} >= {64}
    rng = np.random.default_rng(5)
    fuzz = [(int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(2 ** rng.uniform(0, 24)), int(rng.integers(1, 33)),
             int(rng.integers(1, 33))) for _ in range(300)]
    edges = [(G, W, R, 11, 21) for G, W in ((1, 1), (3, 3), (64, 64)) for R in (1, 63, 64, 65, 255, 256, 257, 4096, 4097, 1 << 19)]
    for s in shapes + clamps + fuzz + edges:
        assert pc.plan(*s).workspace == dll.tl_psf_workspace_bytes(*s), s


# ------------------------------------------------------------------------------------------------------------ sufficient

def _channels(name):
    """Every channel; for many-grids a seeded subset of 64 of its 65535 (the channels differ only in their seeded data, and
    the launch-shape of that case is the GPU test's business), with the first and the last."""
    G, W, R = pc.inputs(name).shape
    if name != "many-grids":
        return [(g, w) for g in range(G) for w in range(W)]
    rng = np.random.default_rng(9)
    flat = np.concatenate(([0, G * W - 1], rng.choice(np.arange(1, G * W - 1), 62, replace=False)))
    return [(int(f) // W, int(f) % W) for f in flat]


@pytest.mark.parametrize("name", list(pc.CASES))
def test_a_float32_emulation_of_the_kernels_stays_within_the_bounds(name):
    a, r = pc.inputs(name), pc.reference(name)
    ch = _channels(name)
    gi, wi = (np.array(v) for v in zip(*ch))
    got = pc.emulate(a, ch)
    line = []
    for what in pc.RESULTS:
        q = pc.ratio(got[what], getattr(r, what)[gi, wi], pc.bound(r, what, a)[gi, wi])
        line.append(f"{what} {q:.3f}")
        assert q <= 1.0, (name, what, q)
        assert (got[what] != 0).any() or name == "dead-channel"
    print(f"PSF-EMU {name}: largest error / bound " + " ".join(line))
    if name == "dead-channel":
        k = ch.index(pc.DEAD_CHANNEL)
        assert not got["hist"][k].any() and not got["gx"][k].any() and not r.hist[pc.DEAD_CHANNEL].any()


@pytest.mark.parametrize("name", ["one-ray", "sub-wave", "reduce-17"])
def test_the_sum_tolerance_of_the_per_grid_gradients_holds_a_float64_sum_and_misses_a_lost_ray(name):
    """The second step of the per-grid gradients: float64 sums of the emulation's own gx, gy in another order (numpy's
    pairwise one), rounded to float32, are within the tolerance of psf_ref.grid_sums; without one ray's term they are not."""
    a = pc.inputs(name)
    G, W, R = a.shape
    got = {k: v.reshape(G, W, R) for k, v in pc.emulate(a).items() if k != "hist"}
    yc32 = (a.y - a.y_centre[:, None, None]).astype(np.float64)
    px, py = a.x_pitch.astype(np.float64), a.y_pitch.astype(np.float64)
    gx, gy = got["gx"].astype(np.float64), got["gy"].astype(np.float64)
    r_live = int(np.flatnonzero(got["gy"][0, 0] * got["gx"][0, 0])[-1])
    for lost in (False, True):
        keep = np.ones(a.shape)
        keep[0, 0, r_live] = 0.0 if lost else 1.0
        got["g_x_pitch"] = (-(gx * a.x * keep).sum(axis=(1, 2)) / px).astype(np.float32)
        got["g_y_pitch"] = (-(gy * yc32 * keep).sum(axis=(1, 2)) / py).astype(np.float32)
        got["g_y_centre"] = (-(gy * keep).sum(axis=(1, 2))).astype(np.float32)
        q = pc.grid_ratios(got, a)
        assert all(v > 1.0 for v in q.values()) if lost else max(q.values()) <= 1.0, (name, lost, q)


# ----------------------------------------------------------------------------------------------------------------- sharp

def _tail(name):
    R = pc.CASES[name][2]
    return (R - 1) // 64 * 64                              # the first ray of the last, ragged batch


def _last_block(name):
    G, W, R, ny, nxh, _, _ = pc.CASES[name]
    pl = pc.plan(G, W, R, nxh, ny)
    assert pl.nbx_fwd > 1
    return ((pl.nbx_fwd - 1) * pc.WAVES * pl.nb * 64, R)


WRONG = [("drop-last", "wave-plus-one", None), ("tail-twice", "block-edge", _tail), ("pitch-w", "sub-wave", None),
         ("rows+4", "block-edge", None), ("block-missing", "reduce-17", _last_block), ("pad-col", "reduce-17", None),
         ("y-first-sign", "sub-wave", None), ("wt-squared", "one-ray", None)]


@pytest.mark.parametrize("variant,name,arg", WRONG, ids=[w[0] for w in WRONG])
def test_a_wrong_evaluation_exceeds_the_bounds(variant, name, arg):
    a, r = pc.inputs(name), pc.reference(name)
    bad = pc.evaluate(a, variant=variant, arg=arg(name) if arg else None)
    q = pc.ratios({k: getattr(bad, k) for k in pc.RESULTS}, r, a)
    print(f"PSF-SHARP {variant} on {name}: " + " ".join(f"{k} {v:.3g}" for k, v in q.items()))
    assert max(q.values()) > 1.0, (variant, name, q)


def test_the_variants_are_all_there():
    assert {w[0] for w in WRONG} == set(ref.VARIANTS)


# ---------------------------------------------------------------------------------- the float32 torch definition of the suite

@pytest.mark.parametrize("name", ["one-ray", "sub-wave", "wave-plus-one"])
def test_the_torch_definition_in_float32_agrees_with_the_reference(name):
    """_hist_torch of tests/test_gpu_psf_fused.py, float32 on the CPU, and its autograd: 1e-5 rel-L2, the project's gradient
    gate."""
    from conftest import rel_l2
    a, r = pc.inputs(name), pc.reference(name)
    t = pc.tensors(a, "cpu")
    for n in pc.LEAVES:
        t[n].requires_grad_(True)
    w = torch.ones_like(t["x"]) if t["weight"] is None else t["weight"].float()
    h = _hist_torch(t["x"], t["y"], w, t["x_pitch"], t["y_pitch"], t["y_centre"], a.nxh, a.ny, a.x_first, a.y_first)
    (h * t["T"]).sum().backward()
    got = dict(zip(pc.RESULTS + pc.GRID, [h.detach()] + [t[n].grad for n in pc.LEAVES]))
    for k, v in got.items():
        e = rel_l2(v.numpy(), getattr(r, k))
        assert v.dtype == torch.float32 and e <= 1e-5, (name, k, e)
