"""
The unrolled aspheric walk-back (trace_bwd_inv_unrolled_kernel<NS, true, PEN>) forms every per-ray address from ONE
wave-uniform chunk offset that advances per ray, and takes its row kinds from the bits of one scalar.  Two things only
show on particular launches:

  * a wrong advance of that offset shows only where a block walks SEVERAL chunks, and the launch plan gives one chunk per
    block below about 2^20 points.  TL_PLAN_FEW is read once per process, so the several-chunks fan runs in fresh child
    processes (tests/walkback_scalar_child.py), one with TL_PLAN_FEW=4 (5 blocks of 7-8 chunks, ragged last chunk) and one
    under the default plan: the lens gradients pass the gates, and the per-ray input gradients -- which no reduction order
    touches; taken from the walk-back kernel through the C entry -- are bit-identical between the two plans, for the
    moment seeds alone, with the uniform penalty seed (aggregate='sum') and with per-ray stack seeds;
  * every way aspheric rows can sit next to each other (a row's own kind and that of the row before it select the row
    code): rows {1,10}, {0}, {10}, {5,6}, {0,1,2,3} (all four hit slots, a chain), no aspheric row at all with kappa /
    poly passed (the aspheric instantiation with no bit set), and {0,1,2,3,4}: more rows than hit slots, which the
    device-side fallback takes, bit-equal to the checkpoint algorithm.

Lens: the 11-row double Gauss (prescriptions.double_gauss); references: the oracle's fp64 autograd, with the gates of
test_gpu_kernel_matrix.py (_grad_errors / _gate, imported).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_kernel_matrix as km
import walkback_scalar_child as wc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_ROWS, F_ROWS, W_ROWS = 777, 3, 2
MASKS = ((1, 10), (0,), (10,), (5, 6), (0, 1, 2, 3), ())
_ORACLE = {}


def _oracle(key, a):
    """fp32 (IEEE sqrt) and fp64 oracle gradients of rms, sumQ and the weighted stack sum on the fan `a` (cached)."""
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import trace_oracle as orc
    S = a["c"].shape[-1]
    names = km._LEAVES + (("kappa", "poly") if a["rows"] else ())
    w = wc.stack_weights(S, a["x"].shape)
    res = {"names": names}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        # z and cy per ray (broadcast to the fan): see test_gpu_kernel_matrix._grad_errors
        lv = {n: (a[n].to(dt).expand(a["x"].shape) if n in km._PER_RAY else a[n].to(dt)).clone().requires_grad_(True)
              for n in names}
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], kind=a["kind"]) if a["rows"] else {}
        o = orc.trace_skew_general(a["x"].to(dt), a["y"].to(dt), lv["z"], a["cx"].to(dt), lv["cy"], lv["c"], lv["t"],
                                   lv["mu"], a["mask"], ieee_sqrt=(dt == torch.float32), aggregate=True, **kw)
        assert o[4].all(), "a ray of the fan does not pass"
        terms = dict(rms=orc.compute_rms2d(o[0], o[1], o[4]), sum=orc.penalty_from_stacks(o[7], S),
                     stk=wc.stack_loss(o[7], w))
        res[tag] = {}
        for t, val in terms.items():
            g = torch.autograd.grad(val, [lv[n] for n in names], retain_graph=True, allow_unused=True)
            res[tag][t] = {n: (torch.zeros_like(lv[n]) if gi is None else gi).double() for n, gi in zip(names, g)}
    # one weight for both penalty forms, from the fp64 oracle: both terms of rms + lam sumQ carry comparable gradient
    res["lam"] = float(res["f64"]["rms"]["c"].norm() / res["f64"]["sum"]["c"].norm())
    _ORACLE[key] = res
    return res


def _check_gate(tag, g, r, a, loss):
    """The lens / launch gradients `g` of rms (+ lam x the penalty form `loss`) against the fp64 oracle."""
    pen, lam = loss != "rms", r["lam"]
    ref = {}
    for t in ("f32", "f64"):
        ref[t] = {n: r[t]["rms"][n] + (lam * r[t][loss][n] if pen else 0.0) for n in r["names"]}
    cancel = km._cancel({n: (r["f64"]["rms"][n], lam * r["f64"][loss][n]) for n in r["names"]}) if pen else None
    got = {n: torch.from_numpy(g[n]).double() for n in r["names"]}
    msg = km._grad_errors(tag, got, ref["f32"], ref["f64"], pen, 1.0, a["rows"], a["c"].shape[-1], cancel)
    if not a["rows"]:
        assert not g["kappa"].any() and not g["poly"].any(), f"{tag}: d/dkappa, d/dpoly of a lens without aspheric rows"
    print(f"{tag}: e64/noise " + ", ".join(msg))


# ------------------------------------------------------------------ several chunks per block
@pytest.fixture(scope="module")
def chunk_runs(tmp_path_factory):
    """The several-chunks fan under TL_PLAN_FEW=4 and under the default plan, one fresh child process each."""
    a = wc.fan(**wc.CHUNK_FAN)
    r = _oracle("chunks", a)
    out = {}
    for plan, few in (("few4", "4"), ("default", None)):
        path = str(tmp_path_factory.mktemp("walkback_scalar") / f"{plan}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("TL_PLAN")}
        if few:
            env["TL_PLAN_FEW"] = few
        cp = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "walkback_scalar_child.py"), path, repr(r["lam"])],
                            capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert cp.returncode == 0, f"{plan}: {cp.stdout[-2000:]}\n{cp.stderr[-4000:]}"
        with np.load(path) as d:
            out[plan] = {k: d[k] for k in d.files}
    return a, r, out


@pytest.mark.parametrize("loss", wc.LOSSES)
def test_several_chunks_per_block_pass_the_gates(chunk_runs, loss):
    a, r, runs = chunk_runs
    for plan in ("few4", "default"):
        g = {n: runs[plan][f"{loss}.{n}"] for n in wc.LEAVES}
        assert runs[plan][f"{loss}.ok"].all()
        _check_gate(f"chunks {plan} {loss}", g, r, a, loss)


@pytest.mark.parametrize("loss", wc.LOSSES)
def test_per_ray_input_gradients_do_not_depend_on_the_launch_plan(chunk_runs, loss):
    _, _, runs = chunk_runs
    for n in ("x", "y"):
        few, dflt = runs["few4"][f"{loss}.cabi.{n}"], runs["default"][f"{loss}.cabi.{n}"]
        assert few.shape == dflt.shape and np.isfinite(few).all() and np.abs(few).max() > 0
        differ = few.view(np.uint32) != dflt.view(np.uint32)
        assert not differ.any(), (f"{loss}: g_{n}_in differs between TL_PLAN_FEW=4 and the default plan on {int(differ.sum())} "
                                  f"of {differ.size} rays, first at flat index {int(np.flatnonzero(differ.ravel())[0])}")


# ------------------------------------------------------------------ row patterns
@pytest.mark.parametrize("loss", wc.LOSSES)
@pytest.mark.parametrize("rows", MASKS, ids=["rows" + "_".join(map(str, m)) if m else "no_rows" for m in MASKS])
def test_row_patterns_pass_the_gates(rows, loss):
    a = wc.fan(P_ROWS, F_ROWS, W_ROWS, rows)
    r = _oracle(rows, a)
    g, inv = wc.run_gpu(a, loss, r["lam"])
    assert inv and g["ok"].all()
    _check_gate(f"rows {rows} {loss}", g, r, a, loss)


@pytest.mark.parametrize("loss", ("rms", "sum"))
def test_more_aspheric_rows_than_hit_slots_fall_back_to_the_checkpoint_kernel(loss):
    from torchoptics_amd import ops
    rows = (0, 1, 2, 3, 4)
    assert len(rows) > ops.ASPH_HIT_SLOTS
    a = wc.fan(P_ROWS, F_ROWS, W_ROWS, rows)
    r = _oracle(rows, a)
    g_inv, inv = wc.run_gpu(a, loss, r["lam"], algo="inverse")
    g_ck, ck_inv = wc.run_gpu(a, loss, r["lam"], algo="checkpoint")
    assert inv and not ck_inv
    for n in wc.LEAVES:
        assert np.array_equal(g_inv[n].view(np.uint32), g_ck[n].view(np.uint32)), f"{loss} d/d{n}: fallback != checkpoint"
    _check_gate(f"rows {rows} {loss} fallback", g_inv, r, a, loss)
