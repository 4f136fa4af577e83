"""The workspace sizers of the three radius-walk operators without a GPU (host functions of csrc/filters.hip, cluster.hip
and iss.hip over the shared carve of csrc/radius_walk.hip): remove_radius_outlier needs the walk's part alone -- the
clamped lengths and, where the call builds grids, grid_carve's block -- and cluster_dbscan and iss_keypoints add their own
(N, P) arrays to it; every array is rounded up to 256 bytes.  The sizes are pinned: a caller's workspace of exactly
*_workspace_bytes is part of the C ABI's contract."""
import pytest

KNOBS = (None, 0, 1)  # POINTOPS_DEBUG=filter_grid / cluster_grid / iss_grid: unset, never a grid, a grid whenever allowed
NS = (1, 3, 65535)
PS = (0, 1, 511, 512, 513, 4096)  # (512 points: from there a cloud gets a grid unasked)

# (knob, N) -> per P of PS the bytes (radius_outlier, cluster, iss), recorded from the library before the three operators
# shared one carve
RECORDED = {
    (None, 1): ((256, 256, 256), (256, 768, 512), (256, 4352, 2304), (125184, 129280, 127232),
                (128768, 133376, 131072), (571904, 604672, 588288)),
    (None, 3): ((256, 256, 256), (256, 768, 512), (256, 12544, 6400), (364032, 376320, 370176),
                (367616, 380416, 374016), (1703936, 1802240, 1753088)),
    (None, 65535): ((524288, 524288, 524288), (524288, 1048576, 786432), (524288, 268431872, 134478080),
                    (7840869888, 8109301248, 7975085568), (7850044928, 8119000576, 7984522752),
                    (37114043648, 39261494528, 38187769088)),
    (0, 1): ((256, 256, 256), (256, 768, 512), (256, 4352, 2304), (256, 4352, 2304), (256, 4864, 2560),
             (256, 33024, 16640)),
    (0, 3): ((256, 256, 256), (256, 768, 512), (256, 12544, 6400), (256, 12544, 6400), (256, 13056, 6656),
             (256, 98560, 49408)),
    (0, 65535): ((524288, 524288, 524288), (524288, 1048576, 786432), (524288, 268431872, 134478080),
                 (524288, 268955648, 134739968), (524288, 269479936, 135002112), (524288, 2147975168, 1074249728)),
    (1, 1): ((256, 256, 256), (65024, 65536, 65280), (125184, 129280, 127232), (125184, 129280, 127232),
             (128768, 133376, 131072), (571904, 604672, 588288)),
    (1, 3): ((256, 256, 256), (176128, 176640, 176384), (363776, 376064, 369920), (364032, 376320, 370176),
             (367616, 380416, 374016), (1703936, 1802240, 1753088)),
    (1, 65535): ((524288, 524288, 524288), (3668387584, 3668911872, 3668649728),
                 (7831173632, 8099081216, 7965127424), (7840869888, 8109301248, 7975085568),
                 (7850044928, 8119000576, 7984522752), (37114043648, 39261494528, 38187769088)),
}


def _aligned(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("knob", KNOBS)
def test_workspace_sizes_of_the_radius_walk_operators(monkeypatch, knob):
    from pytorch3d_pointops_amd import _C

    if knob is None:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    else:
        monkeypatch.setenv("POINTOPS_DEBUG", f"filter_grid={knob},cluster_grid={knob},iss_grid={knob}")
    for N in NS:
        for P, recorded in zip(PS, RECORDED[knob, N]):
            what = f"knob {knob}, N = {N}, P = {P}"
            radius = _C._lib.pointops_radius_outlier_workspace_bytes(N, P)
            cluster = _C._lib.pointops_cluster_workspace_bytes(N, P)
            iss = _C._lib.pointops_iss_workspace_bytes(N, P)
            assert cluster - radius == 2 * _aligned(4 * N * P), what  # parent and rank, int32 (N, P)
            assert iss - radius == _aligned(4 * N * P), what          # the saliency in cell order, float32 (N, P)
            if knob == 0 or P == 0 or (knob is None and P < 512):     # no grid: the clamped lengths, int64 (N,)
                assert radius == _aligned(8 * N), what
            assert (radius, cluster, iss) == recorded, what
