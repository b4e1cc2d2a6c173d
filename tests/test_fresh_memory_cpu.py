"""The fresh-memory harness (tests/fresh_memory.py) without a GPU: it is sharp (an op that leaves one element unwritten, and one
that accumulates into an uncleared workspace, are each reported as a byte difference in exactly that element; a correct op
passes), it covers every way the package allocates uninitialised memory, the strided fill reaches the gaps, and everything is
put back on exit."""
import ast
import glob
import os

import pytest
import torch

import fresh_memory as fm
from torchoptics_amd import imaging, lens_modeling, metrics, ops, paraxial, ray_tracing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
N, SKIPPED = 37, 23


@pytest.fixture
def cpu_workspace(monkeypatch):
    """ops._workspace as it is but for a CPU device (the real one keys its cache by the HIP stream): one cached, growing
    uint8 tensor, allocated through the `torch` name of ops."""
    cache = {}

    def workspace(nbytes, device):
        ws = cache.get("ws")
        if ws is None or ws.numel() < nbytes:
            ws = cache["ws"] = ops.torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        return ws
    monkeypatch.setattr(ops, "_workspace", workspace)
    return cache


# ---- toy ops: written like the entry points of ops.py (the `torch` name of ops, ops._workspace), with numpy-plain bodies
def toy_correct(x):
    out = ops.torch.empty(x.shape, dtype=torch.float32)
    ws = ops._workspace(4 * x.numel(), CPU)[:4 * x.numel()].view(torch.float32)
    ws.copy_(x * 2)                       # writes every word of the scratch it reads
    out.copy_(ws + 1)
    return out, out > 4


def toy_skips_one(x):
    out, flag = toy_correct(x)
    out2 = ops.torch.empty_like(out)
    flag2 = ops.torch.empty(x.shape, dtype=torch.bool)
    keep = torch.arange(x.numel()) != SKIPPED
    out2[keep] = out[keep]
    flag2[keep] = flag[keep]
    return out2, flag2


def toy_accumulates(x):
    out = ops.torch.empty(x.shape, dtype=torch.float32)
    ws = ops._workspace(4 * x.numel(), CPU)[:4 * x.numel()].view(torch.float32)
    ws[:SKIPPED].copy_(x[:SKIPPED])
    ws[SKIPPED + 1:].copy_(x[SKIPPED + 1:])
    ws[SKIPPED] += x[SKIPPED]             # += into scratch that nobody cleared
    out.copy_(ws)
    return out,


def three_runs(op):
    x = torch.linspace(-3, 3, N, dtype=torch.float32)
    runs, soils = [], []
    for byte in fm.FILLS:
        with fm.soiled(byte) as soil:
            runs.append(op(x))
        soils.append(soil)
    return runs, soils


def test_fills_are_zero_a_huge_finite_number_and_nan():
    assert fm.FILLS == (0x00, 0x7F, 0xFF)
    for byte, f32, f64 in ((0x00, 0.0, 0.0), (0x7F, 3.39e38, 1.4e306)):
        raw = torch.full((8,), byte, dtype=torch.uint8)
        assert raw.view(torch.float32)[0].item() == pytest.approx(f32, rel=1e-2)
        assert raw.view(torch.float64)[0].item() == pytest.approx(f64, rel=1e-1)
        assert torch.isfinite(raw.view(torch.float32)).all() and torch.isfinite(raw.view(torch.float64)).all()
    raw = torch.full((8,), 0xFF, dtype=torch.uint8)
    assert torch.isnan(raw.view(torch.float32)).all() and torch.isnan(raw.view(torch.float64)).all()


def test_a_correct_op_passes(cpu_workspace):
    runs, soils = three_runs(toy_correct)
    cmp = fm.same_bytes(runs)
    assert cmp, str(cmp)
    assert cmp.nbytes == N * 4 + N
    for soil in soils:
        assert len(soil.log) == 1 and soil.log[0][1:] == (N * 4, torch.float32)
        assert soil.handouts == 1


def test_an_op_that_leaves_one_element_unwritten_is_flagged_in_that_element(cpu_workspace):
    runs, _ = three_runs(toy_skips_one)
    cmp = fm.same_bytes(runs)
    assert not cmp
    # the float differs under 7F and under FF; the flag byte too (0 / 0x7F / 0xFF -- as a bool all but the first would be True)
    assert cmp.diffs == [(0, 1, [SKIPPED]), (1, 1, [SKIPPED]), (0, 2, [SKIPPED]), (1, 2, [SKIPPED])], str(cmp)
    assert f"first [{SKIPPED}]" in str(cmp)
    flag = runs[2][1]
    assert flag.view(torch.uint8)[SKIPPED].item() == 255
    # ... and any two of the three fills tell it apart, whichever comes first
    assert not fm.same_bytes(runs[1:]) and not fm.same_bytes([runs[2], runs[0]])


def test_an_op_that_accumulates_into_an_uncleared_workspace_is_flagged(cpu_workspace):
    runs, soils = three_runs(toy_accumulates)
    cmp = fm.same_bytes(runs)
    assert not cmp
    assert cmp.diffs == [(0, 1, [SKIPPED]), (0, 2, [SKIPPED])], str(cmp)
    assert torch.isnan(runs[2][0][SKIPPED]) and torch.isfinite(runs[1][0][SKIPPED])
    assert all(s.handouts == 1 for s in soils)


def test_the_workspace_is_refilled_each_time_it_is_handed_out(cpu_workspace):
    with fm.soiled(0x7F) as soil:
        ws = ops._workspace(64, CPU)
        assert (ws == 0x7F).all()
        ws.zero_()
        again = ops._workspace(64, CPU)
        assert again.data_ptr() == ws.data_ptr() and (again == 0x7F).all(), "no state survives an acquisition"
        assert soil.handouts == 2 and soil.log == [], "the cache growing is not an allocation of an op"


def test_same_bytes_compares_none_shapes_and_dtypes():
    a = torch.arange(6, dtype=torch.float32)
    assert fm.same_bytes([{"g": None, "v": a}, {"g": None, "v": a.clone()}])
    assert not fm.same_bytes([{"g": None}, {"g": a}])
    assert not fm.same_bytes([{"g": a}, {"g": None}])
    assert not fm.same_bytes([(a,), (a.double(),)])
    assert not fm.same_bytes([(a,), (a.reshape(2, 3),)])
    assert not fm.same_bytes([{"v": a}, {"w": a}])
    # bits, not values: -0.0 is not +0.0, and one NaN payload is not another; a strided view compares by its logical elements
    assert not fm.same_bytes([torch.tensor([0.0]), torch.tensor([-0.0])])
    nan = torch.tensor([0x7FC00000, 0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert fm.same_bytes([nan[:1], nan[:1].clone()]) and not fm.same_bytes([nan[:1], nan[1:]])
    wide = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    assert fm.same_bytes([wide[:, 1], wide[:, 1].contiguous()])
    assert fm.same_bytes([torch.empty(0), torch.empty(0)]).nbytes == 0


def _allocating_calls():
    """Every attribute call `<something>.empty*(...)` or `<something>.new_empty*(...)` in torchoptics_amd/*.py: {name: [where]}."""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "torchoptics_amd", "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
                name = node.func.attr
                if name.startswith("empty") or name.startswith("new_empty"):
                    found.setdefault(name, []).append(f"{os.path.basename(path)}:{node.lineno}")
    return found


def test_every_uninitialised_allocation_of_the_package_is_one_the_harness_intercepts():
    found = _allocating_calls()
    assert {"empty", "empty_like", "empty_strided"} <= set(found), "the scan sees the allocations of ops.py"
    assert len(found["empty"]) + len(found["empty_like"]) + len(found["empty_strided"]) >= 51
    stray = {n: w for n, w in found.items() if n not in fm.INTERCEPTED}
    assert not stray, f"uninitialised allocations the harness does not soil: {stray}"
    # ... and every module that holds one is a module whose `torch` name the harness replaces
    for name in fm.TORCH_NAMES:
        for where in found.get(name, ()):
            assert where.split(".py:")[0] in fm.MODULES, where
    # the scan itself is sharp: a name torch may grow later is found and refused
    tree = ast.parse("y = torch.empty_permuted((2, 3), (1, 0))\nz = t.new_empty_strided((2,), (1,))")
    names = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
    assert names == {"empty_permuted", "new_empty_strided"} and not names & fm.INTERCEPTED


@pytest.mark.parametrize("byte", fm.FILLS)
def test_every_intercepted_name_fills_and_logs(byte):
    with fm.soiled(byte) as soil:
        made = [ops.torch.empty((3, 5), dtype=torch.float64), imaging.torch.empty_like(torch.ones(7)),
                ray_tracing.torch.empty_strided((2, 3), (8, 1), dtype=torch.float32),
                metrics.torch.empty(4, dtype=torch.bool), paraxial.torch.empty(0), lens_modeling.torch.empty((), dtype=torch.int32),
                torch.ones(5, dtype=torch.int16).new_empty((2, 2))]
        for t in made:
            assert (fm.storage_bytes(t) == byte).all()
        assert soil.log == [(t.untyped_storage().data_ptr(), t.untyped_storage().nbytes(), t.dtype) for t in made]
        assert [n for _, n, _ in soil.log] == [120, 28, 4 * (8 + 3), 4, 0, 4, 8]
        assert all(soil.inside(t) for t in made)
        assert not soil.inside(torch.ones(3)), "a tensor of a torch op lies in no soiled allocation"
        assert soil.inside(made[0][1:, 2:4]) and soil.inside(made[0].t())
    assert made[3].view(torch.uint8).tolist() == [byte] * 4


def test_the_strided_fill_covers_the_gaps_between_rows():
    with fm.soiled(0xFF):
        t = ops.torch.empty_strided((4, 5), (8, 1), dtype=torch.float32)          # three words of padding per row
    raw = fm.storage_bytes(t)
    assert raw.numel() == 4 * (3 * 8 + 5)
    assert (raw == 0xFF).all()
    t.zero_()                                                                     # writes the logical elements only
    words = fm.storage_bytes(t).view(torch.int32)
    gaps = torch.tensor([i * 8 + j for i in range(3) for j in range(5, 8)])
    assert (words[gaps] == -1).all(), "the bytes between the rows were filled"
    assert (t == 0).all()


def _patched_state():
    mods = (ops, imaging, metrics, ray_tracing, paraxial, lens_modeling)
    return ([m.torch for m in mods], ops._workspace, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor),
            [vars(c).get(p) for c in vars(ops).values() if isinstance(c, type) and issubclass(c, torch.autograd.Function)
             for p in ("forward", "backward")],
            ops._host, ops.get_backward_algorithm(), ops.get_default_mode(), ops.ASPH_HIT_SLOTS, ops._warp_image_path)


def test_everything_is_restored_after_the_block_and_after_an_exception():
    before = _patched_state()
    assert all(t is torch for t in before[0])
    with fm.soiled(0x7F):
        assert ops.torch is not torch and ops._workspace is not before[1]
        assert ops.TraceFunction.__dict__["forward"] is not before[4][0]
        assert ops.torch.float32 is torch.float32 and ops.torch.autograd is torch.autograd, "the rest of torch is torch's own"
        ops.set_host_chain("python")
        ops.set_backward_algorithm("checkpoint")
        ops.set_default_mode("fast")
        ops.set_asph_hit_slots(0)
        ops.set_warp_image_grad_path("direct")
    assert _patched_state() == before
    with pytest.raises(ZeroDivisionError):
        with fm.soiled(0xFF):
            ops.set_host_chain("python" if before[5] == "cpp" else "cpp")
            ops.set_default_mode("fast")
            1 / 0
    assert _patched_state() == before
    assert torch.ones(3).new_empty(2).shape == (2,)
    with pytest.raises(ValueError):
        with fm.soiled(256):
            pass
    assert _patched_state() == before


def test_the_nodes_of_ops_are_recorded_with_their_placement():
    class Ctx:
        needs_input_grad = (True,)

    with fm.soiled(0xFF) as soil:
        inside = ops.torch.empty(3)
        rec = soil._recorder(ops.SpotRmsFunction, "backward", lambda ctx: (inside, torch.ones(2), None))
        rec(Ctx())
    assert soil.nodes == [("SpotRmsFunction", "backward", 0, True), ("SpotRmsFunction", "backward", 1, False)]
    assert soil.misplaced() == [("SpotRmsFunction", "backward", 1)]
    assert soil.misplaced(exempt={("SpotRmsFunction", "backward", 1): "a torch multiply"}) == []


def test_the_report_line_has_the_agreed_form():
    line = fm.report_line("ssim", "one_pixel/a", 5, 1, 1, 1234)
    assert line == ("FRESH-MEM ssim one_pixel/a  allocations soiled 5/1  workspace refills 1  bytes compared 1234  "
                    "identical under 00/7F/FF")
