"""The imaging and focus steps (tests/step_cases.py) held to their eager bits where a launch-bound user runs them: on a side
stream, without a host synchronisation, and replayed from a HIP graph.  No tolerance anywhere: every comparison is bit equality
between two ways of running the same step.  Accuracy against fp64 is held by the per-kernel suites and is not repeated here.

The reference of every check is the step run eagerly on the default stream from fresh leaves on input set A, and again on B;
it is computed once per step and shared.

(a) side stream: the step on a new stream, then on a second new one; and two steps that ask for different amounts of the
    kernels' scratch, alternated on one stream.
(b) sync-free: two warm-up calls, then one call under torch.cuda.set_sync_debug_mode("error").  It runs eagerly and reports
    through a Python exception, so it cannot fault.  The mode is documented as not catching every synchronisation: it sees
    the ones PyTorch issues itself (.item(), bool(tensor), nonzero and boolean-mask indexing, a copy from pageable host memory
    as in torch.tensor(..., device=...) or .to(device), .cpu()), not a hipStreamSynchronize a library makes on its own.  The C
    side is covered by reading: csrc/ has no synchronising call on a launch path.
(c) replay: it begins with (b) on the same step -- a step that still synchronises fails there and is never captured, because on
    ROCm a broken capture has shown up as a segfault in hipStreamEndCapture, not as an error -- then graphs.capture_step on
    fresh leaves (one stream: a chain without parallel branches), the static outputs zeroed, replay = A; copy_ B, replay = B;
    copy_ A, two replays = A (nothing carries over: the warp's workspace clear is inside the graph); A's and B's results differ;
    and the host-side call counters of the step's nodes rise during capture and stand still over the replays.
    The whole image-simulation step with Adam is captured in a child process (examples/image_sim_ssim.py --graph).
(d) workspace lifetime: after capture, a larger scratch tensor is forced on the capture stream's cache key; the one the graph
    was recorded with must still be alive (graphs.py, rule 3) and a replay must still give the eager bits.
"""
import gc
import json
import os
import subprocess
import sys
import weakref

import pytest
import torch

import step_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
STEPS = list(step_cases.BUILDERS)
_EAGER = {}


def eager(name):
    """{"A": [...], "B": [...]}: the step's tensors run eagerly on the default stream from fresh leaves, computed once."""
    if name not in _EAGER:
        out = {}
        for which in "AB":
            case = step_cases.build(name, DEV, True)
            case.load(which)
            out[which] = [t.clone() for t in case.step()]
        torch.cuda.synchronize()
        _EAGER[name] = out
    return _EAGER[name]


def assert_bits(name, names, got, want, how):
    assert len(got) == len(want) == len(names)
    for what, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{name} {how}: {what} is {tuple(a.shape)} {a.dtype}"
        assert torch.equal(a, b), f"{name} {how}: {what} does not have the eager bits ({int((a != b).sum())} of {a.numel()} differ)"


def on_new_stream(step):
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = [t.clone() for t in step()]
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    return got


def run_sync_free(step):
    """Two warm-up calls, then one call that raises if PyTorch synchronises with the host; returns that call's tensors."""
    step()
    step()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [t.clone() for t in step()]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return got


# ------------------------------------------------------------------------------------------------------ (a) side stream
@pytest.mark.parametrize("name", STEPS)
def test_a_step_on_a_side_stream_has_the_eager_bits(name):
    ref = eager(name)
    case = step_cases.build(name, DEV, True)
    assert_bits(name, case.names, on_new_stream(case.step), ref["A"], "on a new stream")
    assert_bits(name, case.names, on_new_stream(case.step), ref["A"], "on a second new stream")


def test_two_steps_alternated_on_one_stream_keep_their_own_bits():
    """warp (the fixed-point accumulator, cleared in the scratch) and ms_ssim (the pyramid's partials) ask for different
    amounts of the one scratch tensor of their stream."""
    from torchoptics_amd import ops
    names = ("warp-auto", "ms_ssim")
    cases = {n: step_cases.build(n, DEV, True) for n in names}
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    got = []
    with torch.cuda.stream(s):
        for n in names * 3:
            got.append((n, [t.clone() for t in cases[n].step()]))
        assert len(ops.workspace_of(DEV)) >= 1, "neither step used the scratch of its stream"
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    for n, tensors in got:
        assert_bits(n, cases[n].names, tensors, eager(n)["A"], "alternated on one stream")


# -------------------------------------------------------------------------------------------------------- (b) sync-free
@pytest.mark.parametrize("name", STEPS)
def test_a_warm_step_does_not_synchronise_with_the_host(name):
    ref = eager(name)
    case = step_cases.build(name, DEV, True)
    assert_bits(name, case.names, run_sync_free(case.step), ref["A"], "under the sync debug mode")


def test_the_sync_debug_mode_sees_an_upload_and_a_read_back():
    """The detector detects, and leaves the mode as it found it."""
    t = torch.zeros(3, device=DEV)
    with pytest.raises(RuntimeError):
        run_sync_free(lambda: (t + torch.tensor([1.0, 2.0, 3.0], device=DEV),))
    with pytest.raises(RuntimeError):
        run_sync_free(lambda: (t if bool((t == 0).all()) else t + 1,))
    assert torch.cuda.get_sync_debug_mode() == 0


def test_last_curvature_and_the_aspheric_scale_do_not_synchronise():
    """Two per-step host paths outside the listed steps: paraxial.compute_last_curvature and Lens.scale on an aspheric lens."""
    import yaml_free_lenses as L
    from torchoptics_amd import lens_modeling as lm, paraxial
    lens, _, _ = L.build("cooke", DEV, grad=False)
    c, t, nd = lens.flat_c_but_last, lens.flat_t, lens.flat_nd
    asph = lm.Lens(lens.structure, lens.c, lens.t, lens.nd, lens.v, poly=torch.full((7, 4), 1e-5, device=DEV))
    both = lambda: (paraxial.compute_last_curvature(lens.structure, c, t, nd), asph.scale(2.0).poly)      # noqa: E731
    want = [v.clone() for v in both()]
    last, poly = run_sync_free(both)
    assert last.shape == (7,) and torch.equal(last, want[0]) and torch.equal(last[:6], c) and last[6] != 0
    assert torch.equal(poly, want[1]) and torch.equal(poly, asph.poly / 2.0 ** torch.tensor([3., 5., 7., 9.], device=DEV))


# ----------------------------------------------------------------------------------------------------------- (c) replay
IN_PROCESS = [n for n in STEPS if not n.startswith("image_sim")]


@pytest.mark.parametrize("name", IN_PROCESS)
def test_a_captured_step_replays_the_eager_bits_of_both_input_sets(name):
    from torchoptics_amd import graphs
    ref = eager(name)
    probe = step_cases.build(name, DEV, True)
    assert_bits(name, probe.names, run_sync_free(probe.step), ref["A"], "under the sync debug mode")     # (b) first: no capture of a step that syncs
    one = probe.counts()
    probe.step()
    per_step = {k: v - one[k] for k, v in probe.counts().items()}
    case = step_cases.build(name, DEV, True)                     # fresh leaves: no AccumulateGrad node of another stream
    before = case.counts()
    graph, out = graphs.capture_step(case.step, DEV, warmup=3)
    after = case.counts()
    assert {k: after[k] - before[k] for k in after} == {k: 4 * v for k, v in per_step.items()}, "three warm-up calls and the recording"
    if case.counters:
        assert any(per_step.values())

    def replayed():
        graph.replay()
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    for t in out:
        t.zero_()
    assert_bits(name, case.names, replayed(), ref["A"], "replayed")
    case.load("B")
    assert_bits(name, case.names, replayed(), ref["B"], "replayed on input set B")
    case.load("A")
    replayed()
    assert_bits(name, case.names, replayed(), ref["A"], "replayed twice on input set A again")
    for what, a, b in zip(case.names, ref["A"], ref["B"]):
        assert not torch.equal(a, b), f"{name}: {what} is the same on input sets A and B: the replays show nothing"
    assert case.counts() == after, "a replay went through the host wrappers"


@pytest.mark.parametrize("merit", ["ssim", "ms-ssim"])
def test_the_image_simulation_step_with_adam_replays_the_eager_trajectory(merit):
    """examples/image_sim_ssim.py --graph in a child process, like the other whole-step captures (a capture that goes wrong
    ends the process it runs in): the child runs the step under the sync debug mode on the capture stream first, then records
    it.  Six parameter updates eagerly and as 3 warm-up steps + 3 replays: one trajectory."""
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "image_sim_ssim.py"), "--graph", "--steps", "6", "--log2-pupil", "8",
                         "--fields", "3", "--size", "48", "32", "--merit", merit], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert cp.returncode == 0, f"image_sim_ssim --graph exited with {cp.returncode}\n{cp.stdout[-2000:]}\n{cp.stderr[-3000:]}"
    r = json.loads([ln for ln in cp.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["hip_graph"] and r["sync_free"] and r["replays"] == 3 and r["merit"] == merit
    assert len(r["loss_graph"]) == len(r["loss_eager"]) == 6
    assert r["loss_graph"] == r["loss_eager"], (r["loss_graph"], r["loss_eager"])
    assert r["ssim_graph"] == r["ssim_eager"], (r["ssim_graph"], r["ssim_eager"])
    assert len(set(r["loss_graph"])) == 6, "the loss did not move with every update"


# ----------------------------------------------------------------------------------------------- (d) workspace lifetime
def test_a_captured_trace_keeps_the_scratch_of_the_cpp_host_chain():
    """The trace's scratch is kept by the C++ host chain, in a cache of its own with the same replacement rule: the graph
    holds that tensor too."""
    from torchoptics_amd import graphs, ops
    ext = ops._ext()
    assert ext is not None, "the C++ host chain is not active"
    case = step_cases.build("maps", DEV, True)
    graph, _ = graphs.capture_step(case.step, DEV)
    held = ext.workspace_of(torch.device(DEV).index, graph.stream.cuda_stream)
    assert held is not None, "the trace used no scratch on its capture stream"
    assert any(t.data_ptr() == held.data_ptr() for t in graph.workspace)


def test_the_scratch_a_graph_was_recorded_with_outlives_a_larger_one():
    from torchoptics_amd import graphs, ops
    name = "ms_ssim"                                             # its pyramid partials live in the scratch of ops._workspace
    assert name in step_cases.WORKSPACE
    ref = eager(name)
    case = step_cases.build(name, DEV, True)
    graph, out = graphs.capture_step(case.step, DEV)
    recorded = ops.workspace_of(DEV, graph.stream)
    assert recorded, "the step used no scratch on its capture stream"
    assert {t.data_ptr() for t in graph.workspace} == {t.data_ptr() for t in recorded}
    alive = [weakref.ref(t) for t in recorded]
    pointers = [t.data_ptr() for t in recorded]
    largest = max(t.numel() for t in recorded)
    del recorded
    with torch.cuda.stream(graph.stream):
        grown = ops._workspace(2 * largest, torch.device(DEV))      # the capture stream's cache key now holds a larger tensor
        assert grown.numel() >= 2 * largest and grown.data_ptr() not in pointers
        # what the allocator would hand out in place of a freed scratch tensor, filled with something else
        others = [torch.full((largest,), 0xAB, dtype=torch.uint8, device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    gc.collect()
    assert all(r() is not None for r in alive), "the scratch tensor the graph writes to was freed under it"
    assert all(t.data_ptr() not in pointers for t in others)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_bits(name, case.names, list(out), ref["A"], "replayed after its stream's scratch grew")
    assert all(bool((t == 0xAB).all()) for t in others), "the replay wrote into memory that was no longer its own"
