"""Guarded, poisoned device buffers for the memory contract of include/pointops_amd.h: "inputs are borrowed and never
written; outputs are FULLY written by the call (padding included), so callers may pass uninitialised buffers", scratch
is exactly `*_workspace_bytes()` bytes, and a short or null workspace is POINTOPS_EWORKSPACE.

`contract(monkeypatch, fill)` patches the three names every output and every workspace of pytorch3d_pointops_amd/_C.py
comes through (`_out`, `_out_like`, `_workspace`).  Each buffer it hands out is a view into a larger flat allocation

    [ guard 64 KiB | payload: exactly the requested bytes | guard 64 KiB ]

The guards hold a fixed byte pattern; the payload holds what `fill` says:
    zero    0x00 -- what a fresh block from the driver usually holds, and the padding value of most outputs
    ones    0xFF -- fp32 NaN, int32 / int64 -1: an unwritten element shows, an index read from it stays next to its buffer
    stale   what a SIBLING call (same shapes and arguments, other points, full lengths) left there: `sibling(fn)` runs it
            on fresh buffers, which are then handed back unfilled, in the same order, to the real call; the two calls
            must request the same sequence of (kind, shape, dtype)
The guard is a multiple of 512 bytes, so a payload keeps the alignment torch's allocator gives.

With `short_workspace` ("short" or "null"; both are tried where an error is due) every native call that takes a
workspace is first made with `workspace_bytes - 1` and with a null workspace of the right size
(`assert_too_small_rejected`), on the very buffers of the real call.

This is a helper module, not a conftest: nothing here runs unless a test asks for it."""
import contextlib
import ctypes

import numpy as np
import torch

GUARD = 64 * 1024
assert GUARD % 512 == 0
FILLS = ("zero", "ones", "stale")
# entries whose header documents a fall-back instead of an error ("Without workspace every cloud is scanned"): with
# short_workspace = "short" / "null" THE call itself is made that way, and the test checks its results as usual
FALLBACK_ENTRIES = ("pointops_ball_query",)
EWORKSPACE = -3  # POINTOPS_EWORKSPACE (tests/test_boundary_cpu.py holds the header's codes to the library's)

_PATTERNS = {}


def _pattern(device):
    """The guard bytes: position-dependent (a kernel that writes one repeated value cannot reproduce them), never 0x00
    or 0xFF (the fills)."""
    key = str(device)
    if key not in _PATTERNS:
        i = np.arange(GUARD, dtype=np.int64)
        _PATTERNS[key] = torch.from_numpy((1 + (i * 37 + (i >> 8) * 11) % 253).astype(np.uint8)).to(device)
    return _PATTERNS[key]


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()  # (every stream: the one-call chamfer runs half of its work on a side stream)


def _sync_all():
    """Around a native call, whose arguments are bare pointers: wait for the GPU if this process uses one (the fake
    operators of tests/test_buffer_contract_cpu.py run the same wrappers on CPU tensors)."""
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


class _Buffer:
    def __init__(self, kind, index, shape, dtype, device):
        self.kind, self.shape, self.dtype = kind, tuple(int(s) for s in shape), dtype
        self.name = f"{kind}#{index} {self.shape} {str(dtype).replace('torch.', '')}"
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * item
        self.flat = torch.empty((2 * GUARD + self.nbytes,), dtype=torch.uint8, device=device)
        self.flat[:GUARD] = _pattern(device)
        self.flat[GUARD + self.nbytes:] = _pattern(device)
        self.written = False  # a native call has run since this buffer was handed out

    @property
    def signature(self):
        return (self.kind, self.shape, self.dtype)

    @property
    def payload(self):
        return self.flat[GUARD:GUARD + self.nbytes]

    def fill(self, byte):
        self.payload.fill_(byte)

    def view(self):
        return self.payload.view(self.dtype).view(self.shape)


class Contract:
    def __init__(self, fill, short_workspace=False):
        assert fill in FILLS, fill
        self.fill = fill
        self.short_workspace = short_workspace
        self.buffers = []   # every buffer handed out, in order (the sibling's ARE the real call's under "stale")
        self.rejections = []  # (entry, which workspace argument, "short" | "null") checked by the proxy
        self._queue = None  # "stale": the sibling's buffers still to be handed back
        self._recording = False
        self._watched = []
        self._pending = []  # feature tensors on their way to the next native call through a host array of pointers
        self.inputs_checked = 0  # tensors behind `const` parameters that the wrapped native calls compared

    # ------------------------------------------------------------------------------------------- the three seams
    def _hand_out(self, kind, shape, dtype, device):
        if self._queue is not None:  # the real call of a "stale" run
            assert self._queue, f"stale: the real call requests {kind} {tuple(shape)} {dtype}, the sibling had no more"
            b = self._queue.pop(0)
            want = (kind, tuple(int(s) for s in shape), dtype)
            assert b.signature == want, f"stale: the real call requests {want}, the sibling requested {b.signature}"
            b.written = False
            return b.view()
        b = _Buffer(kind, len(self.buffers), shape, dtype, device)
        # (the sibling's own buffers start from the lucky state, as a first call into fresh memory would)
        b.fill(0xFF if self.fill == "ones" and not self._recording else 0x00)
        self.buffers.append(b)
        return b.view()

    def out(self, *size, dtype=None, device=None):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        return self._hand_out("out", shape, dtype or torch.get_default_dtype(), device or "cpu")

    def out_like(self, t):
        assert t.is_contiguous(), "an output shaped like a non-contiguous tensor"
        return self._hand_out("out", t.shape, t.dtype, t.device)

    def workspace(self, nbytes, dev):
        return self._hand_out("workspace", (int(nbytes),), torch.uint8, dev) if nbytes else None

    # ------------------------------------------------------------------------------------------- the run
    def sibling(self, fn):
        """Run the sibling call of a "stale" run (a no-op under the other fills): its buffers go back to the real call."""
        if self.fill != "stale":
            return
        assert not self.buffers and self._queue is None, "the sibling runs first, once"
        self._recording = True
        try:
            fn()
        finally:
            self._recording = False
        for b in self.buffers:
            _sync(b.flat.device)
        assert self.buffers, "stale: the sibling call requested no buffer"
        self._queue = list(self.buffers)

    def watch(self, **tensors):
        """Snapshot the inputs of the real call (None is skipped) for assert_inputs_unchanged."""
        for name, t in tensors.items():
            if t is not None:
                self._watched.append((name, t, t.detach().clone()))

    def run(self, op, real, sibling_args=None, **watched):
        """op(*sibling_args) as the sibling (under "stale"), then op(*real) with its tensor arguments watched."""
        if self.fill == "stale":
            assert sibling_args is not None, "a stale run needs its sibling's arguments"
            self.sibling(lambda: op(*sibling_args))
        self.watch(**{f"arg{i}": a for i, a in enumerate(real) if torch.is_tensor(a)}, **watched)
        return op(*real)

    def output_bytes(self):
        """[(name, bytes)] of every output handed out, in order: what two runs of a call without atomics must share."""
        return [(b.name, b.payload.cpu().numpy().copy()) for b in self.buffers if b.kind == "out"]

    def _features(self, feature_args):
        """`_C._feature_args` wrapped: the feature tensors reach the library through HOST arrays of pointers, where
        _calls cannot see them, so they are snapshot here for the next native call."""
        def wrapped(x_feats, y_feats):
            if not self._recording:
                self._pending += [(f"{side}_feats[{i}]", t, t.detach().clone())
                                  for side, ts in (("x", x_feats), ("y", y_feats)) for i, t in enumerate(ts)]
            return feature_args(x_feats, y_feats)

        return wrapped

    # ------------------------------------------------------------------------------------------- the checks
    def assert_sequence_consumed(self):
        if self.fill == "stale":
            assert self._queue is not None, "stale: no sibling call was made"
            assert not self._queue, ("stale: the sibling requested more buffers than the real call: "
                                     + ", ".join(b.name for b in self._queue))

    def assert_guards_intact(self):
        assert self.buffers, "no buffer went through the seam: the operator did not allocate through _C._out / _workspace"
        for b in self.buffers:
            _sync(b.flat.device)
            pat = _pattern(b.flat.device)
            for side, lo in (("before", 0), ("after", GUARD + b.nbytes)):
                got = b.flat[lo:lo + GUARD]
                if not torch.equal(got, pat):
                    bad = torch.nonzero(got != pat).flatten()
                    off = int(bad[0])
                    where = f"{off} bytes past its end" if side == "after" else f"{GUARD - off} bytes before its start"
                    raise AssertionError(f"guard {side} {b.name} damaged: first damaged byte {where} "
                                         f"({int(bad.numel())} bytes differ)")

    def assert_inputs_unchanged(self):
        assert self._watched or self.inputs_checked, "no input was watched"
        for name, t, snap in self._watched:
            _sync(t.device)
            a, b = _bits(t), _bits(snap)
            if not torch.equal(a, b):
                off = int(torch.nonzero(a != b).flatten()[0])
                raise AssertionError(f"input {name} {tuple(t.shape)} was written: first changed word at {off}")

    def assert_all_clear(self):
        self.assert_sequence_consumed()
        self.assert_guards_intact()
        self.assert_inputs_unchanged()

    def assert_too_small_rejected(self, call, ws_at, args, what):
        """`call(*args)` with the workspace of argument `ws_at` one byte short, then null at full size: both return
        POINTOPS_EWORKSPACE and launch nothing -- under every fill, the outputs no native call has touched yet keep
        their bytes."""
        fresh = [b for b in self.buffers if b.kind == "out" and not b.written]
        _sync_all()
        before = [b.payload.clone() for b in fresh]
        for label, patch in (("short", {ws_at + 1: args[ws_at + 1] - 1}), ("null", {ws_at: None})):
            tried = [patch.get(i, a) for i, a in enumerate(args)]
            code = call(*tried)
            assert code == EWORKSPACE, f"{what}: {label} workspace (argument {ws_at}) returned {code}, not {EWORKSPACE}"
            self.rejections.append((what, ws_at, label))
        _sync_all()
        for b, snap in zip(fresh, before):
            assert torch.equal(b.payload, snap), f"{what}: a rejected call wrote into {b.name}"
            if self.fill == "ones":
                assert bool((snap == 0xFF).all()), f"{what}: {b.name} did not hold the fill before the call"

    # ------------------------------------------------------------------------------------------- the native calls
    def _calls(self, call_namespace, prototypes):
        """`_C._call` with every entry wrapped: the tensors passed for `const` pointer parameters of the header (idx
        tensors, lengths and workspaces read by the diagnostics included) are snapshot before the call and compared
        bit for bit right after it."""
        import types

        def wrap(name, fn):
            ctypes_ = prototypes["pointops_" + name][1]

            def call(what, dev, *args):
                if self._recording:
                    return fn(what, dev, *args)
                const = [(i, a, a.detach().clone()) for i, (a, ct) in enumerate(zip(args, ctypes_))
                         if torch.is_tensor(a) and ct.startswith("const ")]
                const += [(name_, a, snap) for name_, a, snap in self._pending]
                del self._pending[:]
                fn(what, dev, *args)
                _sync_all()
                for i, a, snap in const:
                    x, y = _bits(a), _bits(snap)
                    if not torch.equal(x, y):
                        off = int(torch.nonzero(x != y).flatten()[0])
                        kind = ctypes_[i] if isinstance(i, int) else "through a host array"
                        raise AssertionError(f"{what}: input {i} ({kind}) {tuple(a.shape)} was written: first changed "
                                             f"word at {off}")
                self.inputs_checked += len(const)

            return call

        return types.SimpleNamespace(**{n: wrap(n, f) for n, f in vars(call_namespace).items()})

    def _proxy(self, lib, signatures):
        """`_C._lib` with every launching entry wrapped: synchronise after the fills, make the short-workspace calls
        first when asked to, and mark the buffers handed out so far as written."""
        contract_, vp, sz = self, ctypes.c_void_p, ctypes.c_size_t

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(lib, name)
                res, argtypes = signatures.get(name, (None, []))
                if res is not ctypes.c_int or not argtypes or argtypes[-1] is not vp or name == "pointops_knn_plan":
                    return fn  # sizers and queries: nothing is launched
                ws_at = [i for i in range(len(argtypes) - 1) if argtypes[i] is vp and argtypes[i + 1] is sz]

                def call(*args):
                    _sync_all()
                    if contract_.short_workspace and not contract_._recording:
                        for i in ws_at:
                            if args[i + 1] > 0 and name in FALLBACK_ENTRIES:
                                args = [{"short": {i + 1: args[i + 1] - 1}, "null": {i: None}}[
                                    contract_.short_workspace].get(j, a) for j, a in enumerate(args)]
                                contract_.rejections.append((name, i, contract_.short_workspace + " (falls back)"))
                            elif args[i + 1] > 0:
                                contract_.assert_too_small_rejected(fn, i, args, name)
                    code = fn(*args)
                    for b in contract_.buffers:
                        b.written = True
                    return code

                return call

        return Proxy()


def _bits(t):
    flat = t.detach().contiguous().view(-1).view(torch.uint8)
    return flat.view(torch.int32) if flat.numel() % 4 == 0 else flat


@contextlib.contextmanager
def contract(monkeypatch, fill, short_workspace=False, module=None, prototypes=None):
    """Patch the buffer seam of `module` (default: pytorch3d_pointops_amd._C) for the duration of the block; the checks
    of the yielded Contract are made after it."""
    if module is None:
        from pytorch3d_pointops_amd import _C as module
    c = Contract(fill, short_workspace)
    saved = {n: getattr(module, n) for n in ("_out", "_out_like", "_workspace", "_lib", "_call", "_feature_args")
             if hasattr(module, n)}
    monkeypatch.setattr(module, "_out", c.out)
    monkeypatch.setattr(module, "_out_like", c.out_like)
    monkeypatch.setattr(module, "_workspace", c.workspace)
    if "_lib" in saved and hasattr(module, "_SIGNATURES"):
        monkeypatch.setattr(module, "_lib", c._proxy(saved["_lib"], module._SIGNATURES))
        if prototypes is not None:  # {symbol: (return type, [parameter types])} of the header (test_boundary_cpu.py)
            monkeypatch.setattr(module, "_call", c._calls(saved["_call"], prototypes))
            monkeypatch.setattr(module, "_feature_args", c._features(saved["_feature_args"]))
    try:
        yield c
    finally:
        for n, v in saved.items():
            monkeypatch.setattr(module, n, v)
