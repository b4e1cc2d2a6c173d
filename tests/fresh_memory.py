"""
Fresh-memory harness: run an op with every uninitialised buffer holding a chosen byte, and compare the bits.

The contract of every entry point of torchoptics_amd ("what every entry point may assume about its buffers"): it
writes every element it returns, and it reads nothing from the shared workspace that the same call did not write.  Outputs,
saved intermediates and the workspace are all `torch.empty*` memory, so a breach shows only when that memory holds something
other than zeros or the previous identical run's answer.  `soiled(byte)` makes it hold `byte`:

  * every `torch.empty`, `torch.empty_like`, `torch.empty_strided` called through the `torch` name of the package's modules,
    and every `Tensor.new_empty`, fills the WHOLE underlying storage of its result with `byte` (the gaps of a strided
    layout included; a tensor without elements has no storage bytes and is only logged);
  * `ops._workspace` refills the workspace tensor with `byte` each time it hands it out, so that no op can carry state in
    it from one acquisition to the next;
  * the forward and backward of every autograd.Function of `ops` is recorded: each tensor a node returns must lie inside an
    allocation the harness soiled (or be listed in the caller's EXEMPT table).

Nothing of the package, of conftest.py or of the pytest settings changes: the patches live in the `with` block and are
taken back on exit, as are ops' host chain, backward algorithm, default mode, hit slots and warp path if the body changed
them.

FILLS:  0x00  fp32 0, fp64 0                   -- what the suite sees on a fresh segment
        0x7F  fp32 3.39e38, fp64 ~1.4e306       -- finite: survives a multiplication by a small weight, exposes += into scratch
        0xFF  NaN, and 255 in a uint8/bool byte -- a NaN survives a multiplication by zero

`same_bytes(runs)` compares what the runs returned as the bytes of their logical elements.
"""
import contextlib
import importlib

import numpy as np
import torch

FILLS = (0x00, 0x7F, 0xFF)

PACKAGE = "torchoptics_amd"
# the modules whose `torch` name is replaced (every module of the package that allocates, and the ones that could)
MODULES = ("ops", "imaging", "metrics", "ray_tracing", "paraxial", "lens_modeling", "dist")
# names intercepted on the `torch` name of MODULES, and on torch.Tensor
TORCH_NAMES = ("empty", "empty_like", "empty_strided")
TENSOR_NAMES = ("new_empty",)
INTERCEPTED = frozenset(TORCH_NAMES + TENSOR_NAMES)
# what soiled() puts back in `ops` on exit
OPS_STATE = ("_host", "_bwd_algo", "_default_mode", "ASPH_HIT_SLOTS", "_warp_image_path")
_INHERITED = object()


def storage_bytes(t):
    """The whole storage under `t` as a flat uint8 tensor (shares memory with t)."""
    st = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),))


def extent(t):
    """(first byte address, one past the last byte address) of the elements `t` addresses; (p, p) without elements."""
    p = t.data_ptr()
    if t.numel() == 0:
        return p, p
    span = sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1
    return p, p + span * t.element_size()


class _Torch:
    """Stands where a module's `torch` name stood: everything is torch's own, except TORCH_NAMES."""

    def __init__(self, soil):
        self.__dict__["_soil"] = soil

    def __getattr__(self, name):
        real = getattr(torch, name)
        if name in TORCH_NAMES:
            return self._soil._allocator(real)
        return real


class Soil:
    """The state of one `soiled(byte)` block: `log` [(data_ptr, nbytes, dtype)] of the soiled allocations in order,
    `handouts` the number of times the workspace was handed out (and refilled), `nodes` [(class, phase, index, inside)] for
    every tensor an autograd node of ops returned."""

    def __init__(self, byte):
        if not 0 <= int(byte) <= 255:
            raise ValueError("the fill is one byte")
        self.byte = int(byte)
        self.log = []
        self.handouts = 0
        self.nodes = []
        self.backward_at = None             # len(log) when the first backward of a node of ops began (None: none ran)
        self._quiet = 0

    # -- allocations
    def soil(self, t):
        """Fill the whole storage under `t` with the byte and log it."""
        st = t.untyped_storage()
        if st.nbytes():
            storage_bytes(t).fill_(self.byte)
        if not self._quiet:
            self.log.append((st.data_ptr(), st.nbytes(), t.dtype))
        return t

    def _allocator(self, real):
        def allocate(*args, **kwargs):
            return self.soil(real(*args, **kwargs))
        return allocate

    def wrap_workspace(self, real):
        def workspace(nbytes, device):
            self._quiet += 1                # (the cache growing is not an allocation of the op)
            try:
                ws = real(nbytes, device)
            finally:
                self._quiet -= 1
            ws.fill_(self.byte)
            self.handouts += 1
            return ws
        return workspace

    # -- placement
    def inside(self, t):
        """Whether every byte `t` addresses lies in one logged allocation (trivially so without elements)."""
        lo, hi = extent(t)
        if lo == hi:
            return True
        return any(p <= lo and hi <= p + n for p, n, _ in self.log)

    def _recorder(self, cls, phase, fn):
        def recorded(*args, **kwargs):
            if phase == "backward" and self.backward_at is None:
                self.backward_at = len(self.log)
            out = fn(*args, **kwargs)
            for k, t in enumerate(out if isinstance(out, tuple) else (out,)):
                if torch.is_tensor(t):
                    self.nodes.append((cls.__name__, phase, k, self.inside(t)))
            return out
        return recorded

    def counts(self):
        """(allocations soiled before the first backward, allocations soiled from then on)."""
        n = len(self.log) if self.backward_at is None else self.backward_at
        return n, len(self.log) - n

    def misplaced(self, exempt=()):
        """The (class, phase, index) of returned tensors outside every soiled allocation, less those in `exempt`."""
        return sorted({n[:3] for n in self.nodes if not n[3] and n[:3] not in exempt})


@contextlib.contextmanager
def soiled(byte, package=PACKAGE, modules=MODULES):
    """Everything uninitialised holds `byte` while the block runs; yields the Soil (log, handouts, nodes)."""
    soil = Soil(byte)
    mods = [importlib.import_module(f"{package}.{m}") for m in modules]
    ops = importlib.import_module(f"{package}.ops")
    undo = []

    def put(obj, name, value):
        # (a class is restored to what its own __dict__ held -- the staticmethod object, or nothing for an inherited name)
        undo.append((obj, name, vars(obj).get(name, _INHERITED) if isinstance(obj, type) else getattr(obj, name)))
        setattr(obj, name, value)

    state = {n: getattr(ops, n) for n in OPS_STATE if hasattr(ops, n)}
    try:
        proxy = _Torch(soil)
        for m in mods:
            if getattr(m, "torch", None) is torch:
                put(m, "torch", proxy)
        for name in TENSOR_NAMES:
            real = getattr(torch.Tensor, name)
            put(torch.Tensor, name, (lambda real: lambda self, *a, **k: soil.soil(real(self, *a, **k)))(real))
        if hasattr(ops, "_workspace"):
            put(ops, "_workspace", soil.wrap_workspace(ops._workspace))
        for cls in list(vars(ops).values()):
            if isinstance(cls, type) and issubclass(cls, torch.autograd.Function) and cls is not torch.autograd.Function:
                for phase in ("forward", "backward"):
                    if phase in cls.__dict__:
                        fn = cls.__dict__[phase]
                        fn = fn.__func__ if isinstance(fn, staticmethod) else fn
                        put(cls, phase, staticmethod(soil._recorder(cls, phase, fn)))
        yield soil
    finally:
        for obj, name, value in reversed(undo):
            if value is _INHERITED:
                delattr(obj, name)
            else:
                setattr(obj, name, value)
        for n, v in state.items():
            setattr(ops, n, v)


# ------------------------------------------------------------------------------------------------------------ comparison
def logical_bytes(t):
    """[numel, itemsize] uint8 on the CPU: the bytes of t's logical elements in C order.  bool goes through a uint8 VIEW
    first, so that an unwritten flag byte shows as 255 and not as True."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.is_complex():
        t = torch.view_as_real(t)
    flat = t.reshape(-1).contiguous().cpu()
    return flat.view(torch.uint8).reshape(flat.numel(), flat.element_size())


class Comparison:
    """The result of same_bytes: true when every run agrees with the first.  `diffs`: [(key, run, [flat element indices])];
    `nbytes`: bytes of one run that were compared."""

    def __init__(self):
        self.diffs = []
        self.nbytes = 0

    def __bool__(self):
        return not self.diffs

    def __str__(self):
        if not self.diffs:
            return f"{self.nbytes} bytes identical"
        return "; ".join(f"{key}: run {run} differs from run 0 "
                         + (what if isinstance(what, str) else f"in {len(what)} element(s), first {what[:8]}")
                         for key, run, what in self.diffs)


def _dtype(t):
    return torch.from_numpy(np.empty(0, t.dtype)).dtype if isinstance(t, np.ndarray) else t.dtype


def _items(run):
    if isinstance(run, dict):
        return list(run.items())
    if torch.is_tensor(run) or isinstance(run, np.ndarray) or run is None:
        return [(0, run)]
    return list(enumerate(run))


def same_bytes(runs):
    """Compare every tensor of runs[1:] with the one under the same key of runs[0], as bytes of their logical elements.
    A run is a dict, a sequence or one tensor; None compares equal to None only."""
    cmp = Comparison()
    first = _items(runs[0])
    want = [(k, None if t is None else (_dtype(t), tuple(t.shape), logical_bytes(t))) for k, t in first]
    cmp.nbytes = sum(w[2].numel() for _, w in want if w is not None)
    for r, run in enumerate(runs[1:], start=1):
        got = _items(run)
        if [k for k, _ in got] != [k for k, _ in first]:
            cmp.diffs.append(("<keys>", r, f"holds {[k for k, _ in got]}, not {[k for k, _ in first]}"))
            continue
        for (key, w), (_, t) in zip(want, got):
            if w is None or t is None:
                if (w is None) != (t is None):
                    cmp.diffs.append((key, r, "one is None, the other is not"))
                continue
            if (_dtype(t), tuple(t.shape)) != w[:2]:
                cmp.diffs.append((key, r, f"is {_dtype(t)} {tuple(t.shape)}, not {w[0]} {w[1]}"))
                continue
            bad = (logical_bytes(t) != w[2]).any(dim=1).nonzero().reshape(-1).tolist()
            if bad:
                cmp.diffs.append((key, r, bad))
    return cmp


def report_line(family, case, n_fwd, n_bwd, refills, nbytes, note=""):
    """The line every case of tests/test_gpu_fresh_memory.py prints (kept in profiles/fresh_memory.txt)."""
    return (f"FRESH-MEM {family} {case}  allocations soiled {n_fwd}/{n_bwd}  workspace refills {refills}  "
            f"bytes compared {nbytes}  identical under 00/7F/FF{note}")
