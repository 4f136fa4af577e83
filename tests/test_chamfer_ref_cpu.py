"""tests/chamfer_ref.py reproduces the reference's chamfer goldens (tests/golden/chamfer.npz): losses and every gradient
of every variant, and the Pointclouds call.  This checks the checker that test_chamfer_float64_gpu.py relies on."""
import numpy as np
import pytest

import cases
from chamfer_ref import CachedKnn, chamfer_distance_ref
from conftest import load_golden


def close(a, b, tol=1e-5):  # the suite's rule (test_gpu_parity.close)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    return a.shape == b.shape and (a.size == 0 or float(np.abs(a - b).max()) <= tol * scale)


@pytest.fixture(scope="module")
def knn(oracle):
    return CachedKnn(oracle)


@pytest.mark.parametrize("v", cases.chamfer_variants(), ids=cases.variant_key)
def test_chamfer_ref_reproduces_golden(knn, v):
    g = load_golden("chamfer")
    key = cases.variant_key(v)
    inp = cases.chamfer_inputs()
    kw = dict(batch_reduction=v["batch_reduction"], point_reduction=v["point_reduction"], norm=v["norm"],
              single_directional=v["single_directional"], abs_cosine=v["abs_cosine"])
    if v["use_weights"]:
        kw["weights"] = inp["w"]
    if v["features"]:
        kw.update(x_features={"normals": inp["xn"]}, y_features={"normals": inp["yn"]}, feature_names=["normals"])
    r = chamfer_distance_ref(knn, inp["x"], inp["y"], inp["xl"], inp["yl"], **kw)
    tags = [tag.replace("lossf/normals", "lossf") for tag, _ in r["outputs"]]
    assert sorted(tags) == sorted(k[len(key) + 1:] for k in g.files
                                  if k.startswith(key + "/") and k.split("/")[-1].startswith("loss"))
    for tag, (_, val) in zip(tags, r["outputs"]):
        assert close(val, g[f"{key}/{tag}"]), (key, tag)
    assert close(r["grad_x"], g[f"{key}/grad_x"]), key
    assert close(r["grad_y"], g[f"{key}/grad_y"]), key
    if v["features"]:
        assert close(r["grad_xf"]["normals"], g[f"{key}/grad_xn"]), key
        assert close(r["grad_yf"]["normals"], g[f"{key}/grad_yn"]), key


def test_chamfer_ref_reproduces_golden_pointclouds(knn):
    """The Pointclouds call of the fixture: ragged lists padded with zeros, default reductions, one feature."""
    g = load_golden("chamfer")
    inp = cases.chamfer_inputs()
    xl, yl = inp["xl"], inp["yl"]
    pad = {}
    for k, lens in (("x", xl), ("xn", xl), ("y", yl), ("yn", yl)):
        a = np.zeros((3, int(lens.max()), 3), np.float32)
        for n in range(3):
            a[n, : lens[n]] = inp[k][n, : lens[n]]
        pad[k] = a
    r = chamfer_distance_ref(CachedKnn(knn.oracle), pad["x"], pad["y"], xl, yl, x_features={"normals": pad["xn"]},
                             y_features={"normals": pad["yn"]}, feature_names=["normals"])
    out = dict(r["outputs"])
    assert close(out["loss"], g["pointclouds/loss"])
    assert close(out["lossf/normals"], g["pointclouds/lossf"])
