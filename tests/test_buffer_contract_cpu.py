"""tests/buffers.py catches what it claims to -- fake operators on CPU tensors, each breaking the buffer contract of
include/pointops_amd.h in one way -- and the package allocates every kernel-written buffer through the seam the helper
patches (an `ast` scan)."""
import ast
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch3d_pointops_amd")


def _module():
    """A stand-in for pytorch3d_pointops_amd._C: the three seam names, as _C.py defines them."""
    return types.SimpleNamespace(
        _out=torch.empty, _out_like=torch.empty_like,
        _workspace=lambda nbytes, dev: torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None)


def _inputs(seed, lengths, N=3, P=40):
    x = torch.rand((N, P), generator=torch.Generator().manual_seed(seed)) + 0.5  # (no zeros: padding is told apart)
    return x, torch.tensor(lengths, dtype=torch.int64)


def _masked_copy(mod, x, lengths, skip_row=None, overrun=None, mutate=False, extra=False):
    """out[n, i] = x[n, i] for i < lengths[n], else 0 -- with one scratch buffer -- and the faults of the tests."""
    N, P = x.shape
    out = mod._out((N, P), dtype=torch.float32, device=x.device)
    ws = mod._workspace(4 * N + 2, x.device)  # (an odd size: the payload is exactly this long)
    if extra:
        mod._out_like(x)
    ws[: 4 * N].view(torch.int32).copy_(lengths.to(torch.int32))
    for n in range(N):
        L = int(ws[: 4 * N].view(torch.int32)[n])
        out[n, :L] = x[n, :L]
        if L < P and n != skip_row:
            out[n, L:] = 0.0
    if overrun == "workspace_end":  # 4 bytes past the scratch
        ws.as_strided((4,), (1,), ws.storage_offset() + ws.numel()).fill_(7)
    if overrun == "output_start":  # 4 bytes before the output
        out.as_strided((1,), (1,), out.storage_offset() - 1).fill_(3.0)
    if mutate:
        x[N - 1, P - 1] += 1.0
    return out


def _want(x, lengths):
    mask = torch.arange(x.shape[1])[None, :] < lengths[:, None]
    return torch.where(mask, x, torch.zeros(()))


def _run(monkeypatch, fill, **faults):
    mod = _module()
    x, lengths = _inputs(1, [40, 17, 0])
    sx, sl = _inputs(2, [40, 40, 40])  # the sibling: another seed, full lengths
    with buffers.contract(monkeypatch, fill, module=mod) as c:
        out = c.run(lambda a, b: _masked_copy(mod, a, b, **faults), (x, lengths), (sx, sl))
    assert mod._out is torch.empty and mod._out_like is torch.empty_like  # the seam is restored
    return c, out, _want(*_inputs(1, [40, 17, 0]))


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_a_correct_operator_passes(monkeypatch, fill):
    c, out, want = _run(monkeypatch, fill)
    assert torch.equal(out, want)
    c.assert_all_clear()
    assert [b.kind for b in c.buffers] == ["out", "workspace"] and c.buffers[1].nbytes == 14


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_an_unwritten_padded_row_shows_under_ones_and_stale_only(monkeypatch, fill):
    c, out, want = _run(monkeypatch, fill, skip_row=1)
    c.assert_all_clear()  # (no guard is touched, no input written: only the values tell)
    equal = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
    assert equal == (fill == "zero"), fill
    if fill == "ones":
        assert bool(torch.isnan(out[1, 17:]).all())
    if fill == "stale":
        assert bool((out[1, 17:] >= 0.5).all())  # live-looking data: the sibling's row


@pytest.mark.parametrize("fill", buffers.FILLS)
@pytest.mark.parametrize("overrun,message", [("workspace_end", r"guard after workspace#1.*0 bytes past its end \(4 bytes"),
                                             ("output_start", r"guard before out#0.*4 bytes before its start \(4 bytes")])
def test_an_overrun_of_four_bytes_is_caught(monkeypatch, fill, overrun, message):
    c, out, want = _run(monkeypatch, fill, overrun=overrun)
    assert torch.equal(out, want)  # (the values do not tell)
    with pytest.raises(AssertionError, match=message):
        c.assert_guards_intact()


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_a_written_input_is_caught(monkeypatch, fill):
    c, out, want = _run(monkeypatch, fill, mutate=True)
    assert torch.equal(out, want)
    c.assert_guards_intact()
    with pytest.raises(AssertionError, match=r"input arg0 \(3, 40\) was written: first changed word at 119"):
        c.assert_inputs_unchanged()


def test_a_sibling_with_another_buffer_sequence_fails(monkeypatch):
    mod = _module()
    x, lengths = _inputs(1, [40, 17, 0])
    for sibling, real, message in (
            (dict(), dict(extra=True), "the sibling had no more"),  # the real call asks for one more
            (dict(extra=True), dict(), "sibling requested more buffers")):  # ... for one fewer
        with buffers.contract(monkeypatch, "stale", module=mod) as c:
            c.sibling(lambda: _masked_copy(mod, x, lengths, **sibling))
            with pytest.raises(AssertionError, match=message) as e:
                _masked_copy(mod, x, lengths, **real)
                c.assert_sequence_consumed()
        assert not isinstance(e.value, pytest.skip.Exception)
    with buffers.contract(monkeypatch, "stale", module=mod) as c:  # the same count, another shape
        c.sibling(lambda: _masked_copy(mod, x[:, :39].contiguous(), lengths))
        with pytest.raises(AssertionError, match=r"stale: the real call requests \('out', \(3, 40\)"):
            _masked_copy(mod, x, lengths)
    with buffers.contract(monkeypatch, "stale", module=mod) as c:  # no sibling at all
        _masked_copy(mod, x, lengths)
    with pytest.raises(AssertionError, match="no sibling call"):
        c.assert_sequence_consumed()


# ------------------------------------------------------------------------------------------------ native calls
# The GPU tests rely on three wrappers of the helper: `_calls` (tensors behind `const` parameters, compared around every
# native call), `_features` (tensors that travel through host arrays of pointers) and `_proxy` (short and null
# workspaces).  Here they wrap a fake library on CPU tensors: masked copy with a 4 * N byte workspace.
_vp, _i64, _sz, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int
_PROTOTYPES = {"pointops_fake": ("int", ["const float*", "const int64_t*", "int64_t", "int64_t", "float*", "void*",
                                         "size_t", "void*"])}


def _native_module(**faults):
    """A stand-in for _C with a `_lib`, a `_call` namespace, `_SIGNATURES` and `_feature_args`; `faults`: ignore_short
    (runs with any workspace), early_write (writes an output, then rejects), write_input, write_feature."""
    tensors = {}  # data_ptr -> tensor: the fake library's view of "device memory"

    class Lib:
        @staticmethod
        def pointops_fake_workspace_bytes(N):
            return 4 * N

        @staticmethod
        def pointops_fake(x, lengths, N, P, out, ws, ws_bytes, stream):
            if faults.get("early_write"):
                tensors[out].view(-1)[0] = 5.0
            if not faults.get("ignore_short") and (ws is None or ws_bytes < 4 * N):
                return buffers.EWORKSPACE
            x, lengths, out = tensors[x], tensors[lengths], tensors[out]
            for n in range(N):
                L = int(lengths[n])
                out[n, :L] = x[n, :L]
                out[n, L:] = 0.0
            if faults.get("write_input"):
                lengths[0] += 1
            return 0

    mod = _module()
    mod._lib, mod._SIGNATURES = Lib, {"pointops_fake_workspace_bytes": (_sz, [_i64]),
                                      "pointops_fake": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _sz, _vp])}

    def fake(what, dev, x, lengths, N, P, out, ws, ws_bytes):
        for t in (x, lengths, out, ws):
            tensors[t.data_ptr()] = t
        code = mod._lib.pointops_fake(x.data_ptr(), lengths.data_ptr(), N, P, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                      None)
        assert code == 0, (what, code)

    mod._call = types.SimpleNamespace(fake=fake)

    def feature_args(x_feats, y_feats):
        if faults.get("write_feature"):
            y_feats[0][0, 0] = -1.0
        return len(x_feats)

    mod._feature_args = feature_args

    def op(x, lengths, feats=()):
        N, P = x.shape
        out = mod._out((N, P), dtype=torch.float32, device=x.device)
        nbytes = mod._lib.pointops_fake_workspace_bytes(N)
        mod._feature_args(list(feats), list(feats))
        mod._call.fake("fake", None, x, lengths, N, P, out, mod._workspace(nbytes, x.device), nbytes)
        return out

    return mod, op


def _native(monkeypatch, fill, feats=(), **faults):
    mod, op = _native_module(**faults)
    x, lengths = _inputs(1, [40, 17, 0])
    with buffers.contract(monkeypatch, fill, short_workspace="short", module=mod, prototypes=_PROTOTYPES) as c:
        c.sibling(lambda: op(*_inputs(2, [40, 40, 40]), [f.clone() for f in feats]))
        out = op(x, lengths, feats)
    return c, out


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_native_call_wrappers_pass_a_correct_entry(monkeypatch, fill):
    c, out = _native(monkeypatch, fill, feats=[torch.ones(2, 2)])
    assert torch.equal(out, _want(*_inputs(1, [40, 17, 0])))
    c.assert_all_clear()
    assert c.inputs_checked == 4  # x, lengths and the feature list, twice (x_feats, y_feats)
    assert c.rejections == [("pointops_fake", 5, "short"), ("pointops_fake", 5, "null")]


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_an_entry_that_runs_on_a_short_workspace_is_caught(monkeypatch, fill):
    with pytest.raises(AssertionError, match=r"pointops_fake: short workspace \(argument 5\) returned 0, not -3"):
        _native(monkeypatch, fill, ignore_short=True)


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_a_rejected_call_that_wrote_an_output_is_caught_under_every_fill(monkeypatch, fill):
    with pytest.raises(AssertionError, match=r"pointops_fake: a rejected call wrote into out#0"):
        _native(monkeypatch, fill, early_write=True)


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_a_written_const_argument_is_caught_at_the_call(monkeypatch, fill):
    with pytest.raises(AssertionError, match=r"fake: input 1 \(const int64_t\*\) \(3,\) was written: first changed word at 0"):
        _native(monkeypatch, fill, write_input=True)


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_a_written_feature_tensor_is_caught_at_the_call(monkeypatch, fill):
    with pytest.raises(AssertionError, match=r"fake: input x_feats\[0\] \(through a host array\) \(2, 2\) was written"):
        _native(monkeypatch, fill, feats=[torch.ones(2, 2)], write_feature=True)


def test_guard_layout():
    assert buffers.GUARD == 64 * 1024 and buffers.GUARD % 512 == 0
    pat = buffers._pattern("cpu")
    assert pat.numel() == buffers.GUARD and int(pat.min()) > 0x00 and int(pat.max()) < 0xFF
    c = buffers.Contract("ones")
    for shape, dtype in (((), torch.float32), ((0, 5), torch.int64), ((3, 7), torch.int64), ((5,), torch.float64)):
        t = c.out(shape, dtype=dtype, device="cpu")
        b = c.buffers[-1]
        assert t.shape == shape and t.dtype == dtype and b.flat.numel() == 2 * buffers.GUARD + b.nbytes
        assert t.numel() == 0 or t.data_ptr() == b.flat.data_ptr() + buffers.GUARD
        if dtype == torch.int64:
            assert bool((t == -1).all())
        elif t.numel():
            assert bool(torch.isnan(t).all())
    assert c.workspace(0, "cpu") is None


# ------------------------------------------------------------------------------------------------ the seam, by ast
_ALLOCATORS = {"empty", "empty_like", "new_empty", "zeros", "zeros_like", "new_zeros"}

# Host-side allocations outside _C.py that no kernel writes: {(file, enclosing function, allocator): (count, reason)}
_HOST_SIDE = {
    ("ops.py", "_like", "new_empty"):
        (1, "the fake (meta) implementations: shapes for torch.compile, never memory a kernel sees"),
    ("ops.py", "_", "empty_like"): (1, "the fake implementation of chamfer_backward"),
    ("ops.py", "_local_frames_grad", "zeros_like"):
        (2, "absent upstream gradients: INPUTS of local_frames_backward that must be zero"),
    ("functions/knn.py", "forward", "new_empty"): (1, "an empty placeholder among the saved tensors"),
    ("functions/chamfer.py", "forward", "new_empty"): (2, "empty placeholders among the saved tensors"),
    ("functions/chamfer.py", "backward", "zeros_like"):
        (1, "an absent upstream gradient: an input of chamfer_backward that must be zero"),
    ("functions/sample_farthest_points.py", "sample_farthest_points", "zeros_like"):
        (1, "the default start indices: an input"),
    ("functions/points_alignment.py", "backward", "zeros_like"): (3, "the gradients of an empty batch: no kernel runs"),
    ("functions/points_alignment.py", "corresponding_points_alignment", "new_zeros"):
        (1, "the weights of an empty list of clouds: an input"),
    ("functions/points_alignment.py", "_report", "zeros_like"): (1, "verbose reporting on the host side"),
    ("functions/points_alignment.py", "_icp_torch", "zeros_like"):
        (1, "the plain-torch ICP route: no kernel of the library writes it"),
}


def _allocations(path):
    """[(enclosing function, allocator attribute)] of every reference to an allocator attribute in a file."""
    found = []

    def visit(node, fn):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            fn = node.name
        if isinstance(node, ast.Attribute) and node.attr in _ALLOCATORS:
            found.append((fn, node.attr))
        for child in ast.iter_child_nodes(node):
            visit(child, fn)

    visit(ast.parse(open(path).read()), "<module>")
    return found


def test_every_kernel_written_buffer_of_the_boundary_comes_through_the_seam():
    """_C.py: torch.empty / torch.empty_like appear exactly three times -- the two aliases and the body of _workspace --
    and nothing is pre-zeroed: every output of the header is allocated with _out / _out_like."""
    path = os.path.join(PKG, "_C.py")
    tree = ast.parse(open(path).read())
    found = _allocations(path)
    assert sorted(found) == [("<module>", "empty"), ("<module>", "empty_like"), ("_workspace", "empty")], found
    assigned = {t.id: ast.unparse(node.value) for node in tree.body if isinstance(node, ast.Assign)
                for t in node.targets if isinstance(t, ast.Name)}
    assert assigned["_out"] == "torch.empty" and assigned["_out_like"] == "torch.empty_like"  # aliases, not wrappers
    workspace = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_workspace")
    inside = [n for n in ast.walk(workspace) if isinstance(n, ast.Attribute) and n.attr in _ALLOCATORS]
    assert len(inside) == 1 and inside[0].attr == "empty"


def test_host_side_allocations_of_the_wrappers_are_the_listed_ones():
    import collections

    files = ["ops.py"] + sorted("functions/" + f for f in os.listdir(os.path.join(PKG, "functions")) if f.endswith(".py"))
    found = collections.Counter((f, fn, attr) for f in files for fn, attr in _allocations(os.path.join(PKG, f)))
    assert dict(found) == {k: n for k, (n, _) in _HOST_SIDE.items()}


def test_short_workspace_code_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "pointops_amd.h")).read()
    assert f"#define POINTOPS_EWORKSPACE ({buffers.EWORKSPACE})" in hdr
