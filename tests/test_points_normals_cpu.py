"""CPU suite of the normals / local-frames feature (functions/points_normals.py, csrc/local_frames.hip): the public
names and their defaults, the argument checks (raised before any device work -- a device call on these CPU tensors
would raise RuntimeError instead), the registered ops and the C ABI entries."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_and_defaults():
    from pytorch3d_pointops_amd import functions
    from pytorch3d_pointops_amd.functions import estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals
    from pytorch3d_pointops_amd.structures import Pointclouds

    assert {"estimate_pointcloud_normals", "estimate_pointcloud_local_coord_frames"} <= set(functions.__all__)
    for fn in (estimate_pointcloud_normals, estimate_pointcloud_local_coord_frames):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:3] == ["pointclouds", "neighborhood_size", "disambiguate_directions"]
        assert sig.parameters["neighborhood_size"].default == 50
        assert sig.parameters["disambiguate_directions"].default is True
        flag = sig.parameters["use_symeig_workaround"]
        assert flag.kind is inspect.Parameter.KEYWORD_ONLY and flag.default is True
    sig = inspect.signature(Pointclouds.estimate_normals)
    assert {k: v.default for k, v in list(sig.parameters.items())[1:]} == {
        "neighborhood_size": 50, "disambiguate_directions": True, "assign_to_self": False}


@pytest.mark.parametrize("fn_name", ["estimate_pointcloud_normals", "estimate_pointcloud_local_coord_frames"])
def test_value_errors_before_device_work(fn_name):
    from pytorch3d_pointops_amd import functions
    from pytorch3d_pointops_amd.structures import Pointclouds

    fn = getattr(functions, fn_name)
    with pytest.raises(ValueError):
        fn(torch.rand(2, 20, 2), neighborhood_size=4)  # D != 3
    with pytest.raises(ValueError, match="float32"):
        fn(torch.rand(2, 20, 3, dtype=torch.float64), neighborhood_size=4)
    with pytest.raises(ValueError, match="float32"):
        fn(torch.rand(2, 20, 3).half(), neighborhood_size=4)
    with pytest.raises(ValueError, match="neighborhood_size"):
        fn(torch.rand(2, 20, 3), neighborhood_size=20)  # lengths[n] <= K: upstream's condition
    with pytest.raises(ValueError, match="neighborhood_size"):
        fn(torch.rand(2, 20, 3))  # the default K = 50
    with pytest.raises(ValueError, match="neighborhood_size"):
        fn(Pointclouds([torch.rand(30, 3), torch.rand(8, 3)]), neighborhood_size=8)  # one short cloud
    with pytest.raises(ValueError, match="float32"):
        fn(Pointclouds([torch.rand(30, 3, dtype=torch.float64)]), neighborhood_size=8)
    with pytest.raises(ValueError, match="float32"):
        Pointclouds([torch.rand(30, 3, dtype=torch.float64)]).estimate_normals(neighborhood_size=8)
    # valid arguments reach the device path, which has no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(torch.rand(2, 20, 3), neighborhood_size=4)


def test_registered_ops():
    from pytorch3d_pointops_amd import ops

    assert {"local_frames", "local_frames_backward"} <= set(ops.registered_ops())


def test_c_abi_entries_declared_and_exported():
    from pytorch3d_pointops_amd import _C

    hdr = open(os.path.join(ROOT, "include", "pointops_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pointops_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ("pointops_local_frames", "pointops_local_frames_backward"):
        assert name in declared
        assert name in _C.exported_symbols()
        assert hasattr(lib, name)


def test_centre_clouds_uses_valid_rows_only():
    from pytorch3d_pointops_amd.functions.points_normals import centre_clouds

    pts = torch.tensor([[[1.0, 2.0, 3.0], [3.0, 2.0, 1.0], [100.0, 100.0, 100.0]]])
    c = centre_clouds(pts, torch.tensor([2]))
    assert torch.equal(c, torch.tensor([[[-1.0, 0.0, 1.0], [1.0, 0.0, -1.0], [0.0, 0.0, 0.0]]]))
