"""Functional API -- same re-exports as the reference's functions/__init__.py:9-17
(chamfer_distance and sample_pdf are imported by module path there too)."""
from .. import ops as _ops  # noqa: F401  registers torch.ops.pointops_amd.* (torch.compile traces through them)
from .ball_query import ball_query
from .cluster import DBSCANClusters, cluster_dbscan, euclidean_clusters
from .filters import (RadiusOutliers, SelectedRows, StatisticalOutliers, mask_to_index, remove_radius_outlier,
                      remove_statistical_outlier, select_rows)
from .fpfh import fpfh_features, mutual_nearest_neighbors, point_pair_features
from .iss import ISSKeypoints, cloud_resolution, iss_keypoints, keypoints_to_padded
from .knn import knn_gather, knn_points
from .knn_in_radius import KNNInRadius, knn_in_radius
from .match import FeatureMatches, match_features
from .mls import MLSSmoothing, smooth_mls
from .packed_to_padded import packed_to_padded, padded_to_packed
from .points_alignment import (ICPSolution, SimilarityTransform, corresponding_points_alignment,
                               iterative_closest_point)
from .plane import PlaneSegmentation, PlaneSet, segment_plane, segment_planes
from .points_normals import estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals
from .ransac import RansacSolution, ransac_alignment
from .registration import RegistrationHistory, RegistrationResult, evaluate_registration, registration_icp
from .sample_farthest_points import sample_farthest_points
from .utils import convert_pointclouds_to_tensor, get_point_covariances, masked_gather, wmean
from .voxel import VoxelDownsample, voxel_downsample, voxels_to_padded

__all__ = [k for k in globals().keys() if not k.startswith("_")]
