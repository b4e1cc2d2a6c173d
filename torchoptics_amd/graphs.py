"""
Whole-step HIP graphs: record one optimisation / loss step (host chain, both trace kernels, autograd, optimiser) once
and replay it -- what makes small workloads GPU-bound instead of launch-bound.

Three rules come with capturing a step that calls `.backward()` on ROCm, two learnt the hard way (a segfault in
hipStreamEndCapture) and the third by reading:

* every autograd node the captured backward touches must have been created ON THE CAPTURE STREAM.  The engine runs a
  leaf's AccumulateGrad node on the stream that node was created on; one left over from an eager step on the default
  stream makes the engine synchronise the capturing stream with the default stream, which ends the capture with a
  segfault.  So: use leaves that have not been through an eager backward (`fresh_leaves`), keep no autograd graph
  alive across steps (re-build `Lens(...)` from the bare leaves inside the step), and warm up on the capture stream;
* nothing inside the step may copy from the host (`torch.tensor(...)`, `.to(device)` of a CPU tensor, `.item()`):
  the package's own constants are cached device tensors for that reason (`lens_modeling.const_tensor`, the tables kept
  on `svola_geometry` / `psf_grid_cells`), and the argument checks of `imaging.radial_map` and `psf_grid_from_fields`
  are decided on host values: pass fields and index maps as host tuples.  tests/test_gpu_steps_graph.py runs every
  step once under `torch.cuda.set_sync_debug_mode("error")` before it captures it;
* what the recorded kernels write must outlive the graph.  The tensors a step allocates while it is recorded live in
  the graph's own memory pool, but the kernels' scratch (`ops._workspace`) is one tensor per (device, stream handle)
  that is REPLACED when a later call on that stream needs a larger one -- and PyTorch hands out stream handles from a
  small pool, so "that stream" may be any later side stream.  The graph holds the raw pointer of the tensor it was
  recorded with; the C++ host chain keeps a cache of the same kind.  `capture_step` therefore returns a graph that keeps
  those tensors alive (`graph.workspace`, next to `graph.stream`): the cache may move on to a larger one, the old one
  is freed with the graph.  A capture made by hand
  (`torch.cuda.graph(...)` around a step) must do the same: keep `ops.workspace_of(device, stream)` with the graph.
"""
import torch

from . import ops

__all__ = ["capture_step", "fresh_leaves"]


def fresh_leaves(*tensors):
    """Detached clones with requires_grad=True: leaves whose AccumulateGrad nodes do not exist yet."""
    out = tuple(t.detach().clone().requires_grad_(True) for t in tensors)
    return out[0] if len(out) == 1 else out


def capture_step(step, device="cuda", warmup=3, stream=None):
    """Warm `step()` up on a side stream, record it into a HIP graph on that stream, return (graph, result).

    The graph carries `graph.stream`, the stream it was recorded on, and `graph.workspace`, the kernels' scratch tensors of
    that stream at the time of recording: the graph keeps them alive for as long as it may be replayed (rule 3 above).

    `step` must be self-contained (zero / drop the gradients it produces, build its autograd graph from bare leaves,
    call backward, optionally the optimiser) and return the tensor(s) to read after each `graph.replay()`; the
    returned `result` is the static output of the recorded step.  Update inputs in place (`leaf.copy_(new)`) between
    replays.  `stream`: the side stream to record on, for a caller who has warmed the step up there already (then `warmup`
    may be 0); by default a new one, and at least one warm-up call."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    cap = torch.cuda.Stream(device) if stream is None else stream
    cap.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(cap):
        for _ in range(max(1 if stream is None else 0, warmup)):
            step()
    torch.cuda.current_stream(device).wait_stream(cap)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        result = step()
    torch.cuda.synchronize(device)
    graph.stream, graph.workspace = cap, ops.workspace_of(device, cap)
    return graph, result
