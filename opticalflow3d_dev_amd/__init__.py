"""opticalflow3d_dev_amd — MI355X-native Lucas–Kanade optical flow.

Drop-in for the hot path of ScientistRachel/OpticalFlow3D_dev
(src/Python/calc_flow.py): ``calc_flow3D``, ``calc_flow2D``, ``process_flow``
(alias ``calc_flow``).  The arithmetic runs as HIP kernels for gfx950 in
``libof3d.so`` (C-ABI: include/of3d.h).
"""

from .analysis import (ContractSpec, FieldSpec, ProjectionSpec, QuiverSpec, RelProfileSpec, SummarySpec,  # noqa: F401
                       centroid_angle, channel_compare, contractility, export_fields, flow_statistics, flow_summary,
                       joint_reliability_mask, largest_component_mask, percentile_threshold,
                       percentile_threshold_device, principal_axes, projection_maps, quiver_sample, quiver_split,
                       reliability_mask, reliability_profile, reliability_thresholds)
from .calc_flow import calc_flow, calc_flow2D, calc_flow2D_fp32, calc_flow3D, calc_flow3D_fp32, process_flow  # noqa: F401
from .taps import make_taps, radii  # noqa: F401

__all__ = ["calc_flow", "calc_flow2D", "calc_flow3D", "process_flow", "calc_flow2D_fp32", "calc_flow3D_fp32",
           "make_taps", "radii", "SummarySpec", "flow_statistics", "flow_summary", "percentile_threshold",
           "percentile_threshold_device", "reliability_mask", "principal_axes", "joint_reliability_mask",
           "channel_compare", "QuiverSpec", "quiver_sample", "quiver_split", "ContractSpec", "contractility",
           "largest_component_mask", "centroid_angle", "RelProfileSpec", "reliability_thresholds",
           "reliability_profile", "FieldSpec", "export_fields", "ProjectionSpec", "projection_maps"]
