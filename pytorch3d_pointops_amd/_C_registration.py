"""Operator boundary of registration_icp (csrc/registration.hip; C ABI: pointops_registration_step and
pointops_registration_workspace_bytes in include/pointops_amd.h, whose REGISTRATION block is the definition).

Beside `_C.py`, not in it, as `_C_filters.py` is: an eager-only building block of functions/registration.py, not a
registered operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output
seam -- looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees these calls too.  There is
no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

ESTIMATIONS = {"point_to_point": 0, "point_to_plane": 1}
# fp64 words per cloud of the optional `moments` output: A (21), b (6), c, sum d2 -- or the 24 alignment moments, 3 zeros,
# c, sum d2 -- then the x (6) the point-to-plane solve returned
MOMENTS = 35
STATE_WORDS = 16  # fp64 words of a cloud's state: R (9), T (3), prev_fitness, prev_rmse, 2 spare
RUNNING, CONVERGED, DEGENERATE = 2, 0, 1  # status of a cloud
DEGENERATE_PIVOT = 1e-10  # kIcpDegeneratePivot of csrc/icp_plane.h
MIN_INLIERS = {"point_to_point": 3, "point_to_plane": 6}
SEARCHES = ("exact", "bounded")
SEARCH_BOUNDED = -2  # POINTOPS_REGISTRATION_SEARCH_BOUNDED of the header: no version of knn_points


class RegistrationState:
    """Device buffers of one registration_icp run and the stepping primitive over them, modelled on `_C.IcpState`.  The
    run OWNS its search workspace -- the grid over the target cloud `Y` is built by the first step and reused by the
    later ones -- and never touches the grid cache of `_C` or its statistics.  `Y`, `normals` and the lengths must not
    be written between steps.  History entry i lives in R[i], T[i], fitness[i], inlier_rmse[i]; everything else holds
    the state after the last step.  Every buffer is uninitialised until the first step, which writes all of them."""

    def __init__(self, X_init, Y, normals, lengths_x, lengths_y, R_init, T_init, max_correspondence_distance: float,
                 estimation: str, max_steps: int, relative_fitness: float, relative_rmse: float,
                 want_moments: bool = False, reuse_grid: bool = True, search: str = "exact"):
        if search not in SEARCHES:
            raise ValueError(f"registration: search is one of {SEARCHES}, got {search!r}")
        dev = _C._require_gpu(X_init, Y, normals, lengths_x, lengths_y, R_init, T_init)
        self.X_init, self.Y, self.normals = _C._f32c(X_init, "source"), _C._f32c(Y, "target"), \
            _C._f32c(normals, "target_normals")
        self.lengths_x, self.lengths_y = _C._i64c(lengths_x, "lengths_x"), _C._i64c(lengths_y, "lengths_y")
        self.R_init, self.T_init = _C._f32c(R_init, "R"), _C._f32c(T_init, "T")
        if estimation not in ESTIMATIONS:
            raise RuntimeError(f"registration: estimation is one of {sorted(ESTIMATIONS)}")
        if self.X_init.dim() != 3 or self.Y.dim() != 3:
            raise RuntimeError("registration: source and target must be 3-dimensional")
        N, P1, D = self.X_init.shape
        P2 = self.Y.shape[1]
        if (self.Y.shape[0] != N or self.Y.shape[2] != D or D != 3 or min(N, P1, P2) < 1
                or self.lengths_x is None or self.lengths_x.shape != (N,)
                or self.lengths_y is None or self.lengths_y.shape != (N,)
                or (self.normals is not None and self.normals.shape != self.Y.shape)
                or (self.normals is None and estimation == "point_to_plane")
                or (self.R_init is None) != (self.T_init is None)
                or (self.R_init is not None and (self.R_init.shape != (N, 3, 3) or self.T_init.shape != (N, 3)))):
            raise RuntimeError("registration: need source (N,P1,3), target (N,P2,3) with N, P1, P2 >= 1, lengths (N,), "
                               "target_normals (N,P2,3) for point_to_plane, and R (N,3,3) with T (N,3) or neither")
        max_steps = int(max_steps)
        if max_steps < 1:
            raise RuntimeError("registration: max_steps has to be >= 1")
        self.dev, self.shape = dev, (N, P1, P2)
        self.estimation = ESTIMATIONS[estimation]
        self.r_max = float(max_correspondence_distance)
        self.thr = (float(relative_fitness), float(relative_rmse))
        self.steps = 0
        out = _C._out
        self.Xt = out((N, P1, 3), dtype=torch.float32, device=dev)
        self.state = out((N, STATE_WORDS), dtype=torch.float64, device=dev)
        self.status = out((N,), dtype=torch.int32, device=dev)
        self.iterations = out((N,), dtype=torch.int32, device=dev)
        self.idx = out((N, P1), dtype=torch.int64, device=dev)
        self.dists = out((N, P1), dtype=torch.float32, device=dev)
        self.correspondences = out((N, P1), dtype=torch.int64, device=dev)
        self.num_correspondences = out((N,), dtype=torch.int64, device=dev)
        self.R = out((max_steps, N, 3, 3), dtype=torch.float32, device=dev)
        self.T = out((max_steps, N, 3), dtype=torch.float32, device=dev)
        self.fitness = out((max_steps, N), dtype=torch.float32, device=dev)
        self.inlier_rmse = out((max_steps, N), dtype=torch.float32, device=dev)
        self.all_frozen = out((1,), dtype=torch.int32, device=dev)
        self.moments = out((N, MOMENTS), dtype=torch.float64, device=dev) if want_moments else None
        # asked once per run (-1 unless a debug knob forces the grid) and passed to every step: the search workspace
        # step 0 builds belongs to one kernel family
        # search="bounded": the K = 1 knn_in_radius with the run's radius on a workspace of ITS size; the target side of
        # its search structure is kept from step 0 on in the same way (a call too small for a grid has none to keep)
        if search == "bounded":
            self.search_version = SEARCH_BOUNDED
            self.knn_ws, self.knn_ws_bytes = _C._scratch(dev, _C._lib.pointops_knn_in_radius_workspace_bytes, N, P1, P2,
                                                         3, 1)
            self.uses_grid = True
        else:
            self.search_version = version = _C._lib.pointops_registration_search_version()
            self.knn_ws, self.knn_ws_bytes = _C._scratch(dev, _C._lib.pointops_knn_workspace_bytes, N, P1, P2, 3, 1,
                                                         version)
            self.uses_grid = bool(_C._lib.pointops_knn_uses_grid(N, P1, P2, 3, 1, version))
        self.ws, self.ws_bytes = _C._scratch(dev, _C._lib.pointops_registration_workspace_bytes, N, P1)
        self.reuse_grid = bool(reuse_grid) and self.uses_grid

    def step(self, update: bool = True) -> None:
        """Enqueue one step (no synchronisation).  `update=False`: the evaluate-only step."""
        N, P1, P2 = self.shape
        i = self.steps
        if i >= self.R.shape[0]:
            raise RuntimeError("registration: more steps than max_steps")
        _C._call.registration_step(
            "registration_step", self.dev, self.X_init, self.Y, self.normals, self.lengths_x, self.lengths_y,
            self.R_init, self.T_init, N, P1, P2, self.r_max, self.thr[0], self.thr[1], self.estimation, bool(update),
            i == 0, 1 if (self.reuse_grid and i > 0) else 0, self.search_version, self.Xt, self.state, self.status,
            self.iterations, self.idx, self.dists, self.correspondences, self.num_correspondences, self.R[i],
            self.T[i], self.fitness[i], self.inlier_rmse[i], self.all_frozen, self.moments, self.knn_ws,
            self.knn_ws_bytes, self.ws, self.ws_bytes)
        self.steps = i + 1

    def repeat_last_entry(self) -> None:
        """Fill the history entries no step has written with the last written one: what the steps a host loop skipped
        after `all_frozen` would have written."""
        i = self.steps
        if 0 < i < self.R.shape[0]:
            for h in (self.R, self.T, self.fitness, self.inlier_rmse):
                h[i:] = h[i - 1]
