"""The registered operators (pytorch3d_pointops_amd/ops.py) against the operator boundary `_C`, their schemas, and
their fake (meta) implementations on every sample of tests/registered_ops_cases.py -- fake CUDA tensors under
FakeTensorMode need the built library (for `_C`'s import) but no device."""
import inspect

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.symbolic_shapes import ShapeEnv

import registered_ops_cases as roc
from pytorch3d_pointops_amd import _C, ops

# `_C` callables that launch kernels and are NOT registered operators, each with the reason.
NOT_REGISTERED = {
    "knn_grid_fallback_counts": "diagnostics of the grid search for tools and benchmarks: never part of a model",
    "knn_grid_stats": "diagnostics of the grid search for tools and benchmarks: never part of a model",
    "chamfer_pair_forward": "eager-only fusion of both directions; traced graphs compose knn_points_idx, "
                            "gather_neighbors and chamfer_reduce instead (functions/chamfer.py)",
    "chamfer_pair_backward": "the backward of chamfer_pair_forward: eager only, like it",
    "IcpState": "iterative_closest_point owns device state across a host loop that reads a convergence flag back "
                "every iteration: not traceable and not differentiable",
}


def _schema(name):
    return getattr(torch.ops.pointops_amd, name).default._schema


def _fake_to(a):
    return torch.empty(a.shape, dtype=torch.from_numpy(np.empty(0, a.dtype)).dtype, device="cuda")


def _fake_to_outside(a):
    return torch.empty(a.shape, dtype=torch.from_numpy(np.empty(0, a.dtype)).dtype, device="meta")


def _launches(obj) -> bool:
    src = inspect.getsource(obj)
    return "_call." in src or "_grid_diagnostics(" in src


def test_table_covers_the_registered_ops():
    assert set(roc.TABLE) == set(ops.registered_ops())
    assert len(ops.registered_ops()) == 18
    for name, op in roc.TABLE.items():
        assert op.samples(_fake_to_outside), name


def test_every_op_is_a_C_callable_with_the_same_parameters():
    for name in ops.registered_ops():
        fn = getattr(_C, roc.TABLE[name].c_name or name)
        assert callable(fn) and _launches(fn), name
        c_params = [p for p in inspect.signature(fn).parameters if p not in roc.C_ONLY_PARAMETERS.get(name, ())]
        assert c_params == [a.name for a in _schema(name).arguments], name
    for name, extra in roc.C_ONLY_PARAMETERS.items():
        assert extra <= set(inspect.signature(getattr(_C, name)).parameters), name


def test_every_launching_C_callable_is_registered_or_listed():
    public = {n: o for n, o in vars(_C).items() if not n.startswith("_") and (inspect.isfunction(o) or inspect.isclass(o))
              and getattr(o, "__module__", None) == _C.__name__}
    launching = {n for n, o in public.items() if _launches(o)}
    assert launching == set(ops.registered_ops()) | set(NOT_REGISTERED)
    assert not set(NOT_REGISTERED) & set(ops.registered_ops())


def test_schemas():
    for name in ops.registered_ops():
        schema, op = _schema(name), roc.TABLE[name]
        written = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
        assert written == roc.MUTATED_ARGUMENTS.get(name, set()), name
        optional = {a.name for a in schema.arguments if str(a.type).startswith("Optional")}
        assert optional == roc.OPTIONAL_ARGUMENTS.get(name, set()), name
        samples = op.samples(_fake_to_outside)
        for i, arg in enumerate(schema.arguments):
            absent = {s[i] is None for s in samples.values()}
            assert absent == ({True, False} if arg.name in optional else {False}), (name, arg.name)
        # return arity: one Tensor per documented output, or ONE Tensor[] for the two list-returning backward passes
        want = op.outputs(*next(iter(samples.values())))
        kinds = [str(r.type) for r in schema.returns]
        if want is None:
            assert kinds == [], name
        elif name in ("chamfer_backward", "points_alignment_backward"):
            assert kinds == ["List[Tensor]"], name
        else:
            assert kinds == ["Tensor"] * len(want), name


@pytest.mark.parametrize("name", sorted(roc.TABLE))
def test_fake_outputs_are_the_documented_ones(name):
    op = roc.TABLE[name]
    with FakeTensorMode(shape_env=ShapeEnv()):
        for sample, args in op.samples(_fake_to).items():
            want = op.outputs(*args)
            got = getattr(torch.ops.pointops_amd, name)(*args)
            if want is None:
                assert got is None, (name, sample)
                continue
            got = list(got) if isinstance(got, (tuple, list)) else [got]
            assert len(got) == len(want), (name, sample)
            for t, (shape, dtype) in zip(got, want):
                assert t.dtype == dtype and t.device.type == "cuda" and t.device == args[0].device, (name, sample)
                assert len(t.shape) == len(shape), (name, sample)
                unbacked = 0
                for have, size in zip(t.shape, shape):
                    if size == roc.UNBACKED:
                        assert isinstance(have, torch.SymInt) and not have.node.has_hint(), (name, sample)
                        unbacked += 1
                    else:
                        assert isinstance(have, int) and have == size, (name, sample, tuple(t.shape), shape)
                if not unbacked:
                    assert t.is_contiguous(), (name, sample)
                else:
                    assert unbacked == 1 and t.stride(1) == 1, (name, sample)


def test_fps_fake_has_one_unbacked_dimension():
    with FakeTensorMode(shape_env=ShapeEnv()):
        args = roc.TABLE["sample_farthest_points"].samples(_fake_to)["ragged_unknown_max"]
        out = torch.ops.pointops_amd.sample_farthest_points(*args)
        assert out.shape[0] == roc.N and isinstance(out.shape[1], torch.SymInt) and not out.shape[1].node.has_hint()
        known = torch.ops.pointops_amd.sample_farthest_points(*args[:4], 40)
        assert tuple(known.shape) == (roc.N, 40)
