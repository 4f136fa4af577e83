"""The cases of tests/test_moment_passes_gpu.py and of tools/record_moment_passes.py: every output of the per-cloud moment
passes (points_alignment, IcpState, RegistrationState) at the smallest shapes where their summation order can show.

Every case is N = 3 clouds of lengths (0, 1, P).  P = 1, 255, 256, 257 sit around one block of 256 threads, 2049 is the
first size with two blocks of partials per cloud and 65 537 the first at which the 32 blocks are all there and every
thread walks twice.  Inputs come from synth seeds, so a recording holds outputs only: per case one byte string, the
`whole` fields in their own dtypes followed by a 16-byte blake2b digest of each `digest` field, in the order compute()
returns them.
"""
import hashlib

import numpy as np
import torch

from pytorch3d_pointops_amd import synth

SIZES = (1, 255, 256, 257, 2049, 65537)
STEPS = 3
R_MAX = 0.04  # registration: some rows of the perturbed target fall outside, so the sums are over a trimmed set


def case_names():
    names = [f"alignment-D{D}-{'idx' if idx else 'rows'}-{'weights' if w else 'ones'}-P{P}"
             for P in SIZES for D in (2, 3) for idx in (False, True) for w in (False, True)]
    names += [f"icp-P{P}" for P in SIZES]
    names += [f"registration-{est}-P{P}" for P in SIZES for est in ("point_to_plane", "point_to_point")]
    return names


def _seed(name):
    return int.from_bytes(hashlib.blake2b(name.encode(), digest_size=4).digest(), "little")


def _lengths(P, dev):
    return torch.tensor([0, 1, P], dtype=torch.int64, device=dev)


def _G(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _moved(seed, X):
    """X under a small rigid motion plus noise of up to 0.04 per coordinate, fp32"""
    D = X.shape[-1]
    c, s = np.float32(np.cos(0.05)), np.float32(np.sin(0.05))
    R = np.eye(D, dtype=np.float32)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = c, s, -s, c
    noise = (synth.uniform_f32(seed, X.shape) - np.float32(0.5)) * np.float32(0.08)
    return (X @ R + np.float32(0.01) + noise).astype(np.float32)


def _alignment(name, dev):
    from pytorch3d_pointops_amd import _C

    _, Dn, how, wn, Pn = name.split("-")
    D, P, seed = int(Dn[1:]), int(Pn[1:]), _seed(name)
    X = synth.uniform_f32(seed, (3, P, D))
    Y = _moved(seed + 1, X)
    idx = _G(dev, synth.randint(seed + 2, 0, P - 1, (3, P))) if how == "idx" else None
    w = _G(dev, synth.uniform_f32(seed + 3, (3, P))) if wn == "weights" else None
    Xd, Yd, lengths = _G(dev, X), _G(dev, Y), _lengths(P, dev)
    R, T, s, sing, moments = _C.points_alignment(Xd, Yd, idx, lengths, w, True, False, 1e-9, want_moments=True)
    grad_moments = _G(dev, synth.uniform_f32(seed + 4, tuple(moments.shape)).astype(np.float64) - 0.5)
    gX, gY, gw = _C.points_alignment_backward(Xd, Yd, lengths, w, grad_moments)
    whole = {"R": R, "T": T, "s": s, "singular_values": sing, "moments": moments}
    digest = {"grad_X": gX, "grad_Y": gY}
    if gw is not None:
        digest["grad_w"] = gw
    return whole, digest


def _icp(name, dev):
    from pytorch3d_pointops_amd import _C

    P, seed = int(name.split("-P")[1]), _seed(name)
    X = synth.uniform_f32(seed, (3, P, 3))
    Xd, Yd, lengths = _G(dev, X), _G(dev, _moved(seed + 1, X)), _lengths(P, dev)
    state = _C.IcpState(Xd, Xd.clone(), Yd, lengths, lengths, STEPS, True, False, 1e-6)
    whole = {}
    for i in range(STEPS):
        state.step()
        whole[f"rmse[{i}]"] = state.rmse.clone()
    whole.update({"R": state.R, "T": state.T, "s": state.s, "converged": state.converged})
    return whole, {"Xt": state.Xt, "idx": state.idx}


def _registration(name, dev):
    from pytorch3d_pointops_amd import _C_registration

    _, est, Pn = name.split("-")
    P, seed = int(Pn[1:]), _seed(name)
    X = synth.uniform_f32(seed, (3, P, 3))
    Xd, Yd, lengths = _G(dev, X), _G(dev, _moved(seed + 1, X)), _lengths(P, dev)
    normals = _G(dev, synth.unit_normals(seed + 2, (3, P, 3)))
    state = _C_registration.RegistrationState(Xd, Yd, normals if est == "point_to_plane" else None, lengths, lengths,
                                              None, None, R_MAX, est, STEPS, 1e-6, 1e-6, want_moments=True)
    whole = {}
    for i in range(STEPS):
        state.step(update=True)
        whole[f"moments[{i}]"] = state.moments.clone()
    whole.update({"R": state.R, "T": state.T, "fitness": state.fitness, "inlier_rmse": state.inlier_rmse,
                  "status": state.status, "iterations": state.iterations,
                  "num_correspondences": state.num_correspondences, "state": state.state})
    return whole, {"Xt": state.Xt, "correspondences": state.correspondences}


def compute(name, dev):
    """[(field, bytes)] of one case: the whole fields as their bytes, then the digests"""
    fn = {"alignment": _alignment, "icp": _icp, "registration": _registration}[name.split("-")[0]]
    whole, digest = fn(name, dev)
    torch.cuda.synchronize(dev)
    raw = lambda t: np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()  # noqa: E731
    return [(k, raw(v)) for k, v in whole.items()] + \
        [(k + " (digest)", hashlib.blake2b(raw(v), digest_size=16).digest()) for k, v in digest.items()]
