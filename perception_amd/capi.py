"""ctypes binding of libcuboid_hip.so (the C-ABI declared in include/cuboid_hip.h).

This is the only way Python reaches the HIP path; there is no CPU fallback.  Loading
fails loudly when the shared library has not been built (run `python -c "import
__graft_entry__ as g; g.build()"` or `make -C perception_amd/csrc`).
"""
import ctypes as C
import os

import numpy as np

CD_ABI_VERSION = 4
CD_MAX_TEMPLATES = 8
CD_MAX_CLUSTERS_PER_FRAME = 8
CD_FRAME_MORE_CLUSTERS = 1
CD_FRAME_SURFACE_GUESS = 2
CD_FRAME_CLUSTER_GUESS = 4

CD_OK = 0
CD_ERR_INVALID_ARG = -1
CD_ERR_CAPACITY = -2
CD_ERR_DEVICE = -3
CD_ERR_NO_MODEL = -4
CD_ERR_FEW_CORRESPONDENCES = -5
CD_ERR_LEAF_TOO_SMALL = -6
CD_ERR_NO_TEMPLATE = -7

LIB_PATH = os.environ.get("CUBOID_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libcuboid_hip.so")

# every symbol include/cuboid_hip.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "cd_default_params", "cd_abi_version", "cd_struct_size", "cd_create", "cd_destroy", "cd_last_error",
    "cd_set_template", "cd_crop_voxel", "cd_segment_plane", "cd_extract", "cd_surface_frame", "cd_bbox_filter", "cd_cluster", "cd_icp",
    "cd_process_batch", "cd_process_frame", "cd_process_batch_device", "cd_get_cluster_results", "cd_pose_to_position_quaternion",
    "cd_bbox_corners", "cd_get_timing", "cd_get_frame_cloud", "cd_get_cluster_points", "cd_ground_plane", "cd_set_frame_guesses",
    "cd_template_lattice_faces", "cd_template_nearest", "cd_lattice_detect", "cd_lattice_axes", "cd_passthrough",
    "cd_default_depth_camera", "cd_depth_to_cloud", "cd_process_depth_batch", "cd_process_depth_batch_device",
    "cd_set_icp_max_correspondence_distance", "cd_get_icp_max_correspondence_distance", "cd_icp_correspondence_threshold",
    "cd_surface_batch", "cd_surface_guess", "cd_set_surface_distance_threshold", "cd_get_surface_distance_threshold",
    "cd_get_surface_results",
    "cd_default_color_gate_params", "cd_color_bbox_batch", "cd_color_bbox_batch_device", "cd_set_frame_bboxes", "cd_set_bbox_source",
    "cd_get_bbox_source", "cd_get_frame_bboxes",
    "cd_default_overlay_params", "cd_overlay_project", "cd_draw_boxes_batch", "cd_draw_boxes_batch_device", "cd_draw_last_results",
    "cd_draw_last_results_device",
    "cd_default_verify_params", "cd_verify_struct_size", "cd_verify_pixel", "cd_verify_box_host", "cd_verify_boxes_batch",
    "cd_verify_boxes_batch_device", "cd_verify_last_results", "cd_verify_last_results_device",
    "cd_default_color_camera", "cd_color_camera_struct_size", "cd_texture_project", "cd_depth_to_cloud_mapped",
    "cd_process_depth_batch_mapped", "cd_process_depth_batch_mapped_device",
    "cd_shape_frame_struct_size", "cd_shape_frame_host", "cd_shape_frames", "cd_template_shape_frame", "cd_shape_guess",
    "cd_get_cluster_shape_frames",
    "cd_icp_solve_batch",
    "cd_label_points_last", "cd_label_points_last_device", "cd_label_depth_last", "cd_label_depth_last_device",
    "cd_default_label_palette", "cd_label_struct_size", "cd_tint_labels_batch", "cd_tint_labels_batch_device",
    "cd_set_outlier_filter", "cd_get_outlier_filter", "cd_get_outlier_stats", "cd_outlier_filter",
    "cd_set_icp_plane_weight", "cd_get_icp_plane_weight", "cd_get_cluster_plane_stats", "cd_icp_plane_solve_host",
    "cd_set_icp_coarse", "cd_get_icp_coarse", "cd_icp_coarse_struct_size", "cd_icp_coarse_subsample", "cd_get_cluster_coarse_stats",
    "cd_set_icp_median_rejection", "cd_get_icp_median_rejection", "cd_icp_reject_struct_size", "cd_get_cluster_reject_stats",
    "cd_icp_median_threshold",
    "cd_set_icp_reciprocal", "cd_get_icp_reciprocal", "cd_icp_recip_struct_size", "cd_get_cluster_recip_stats", "cd_icp_reciprocal_mask",
    "cd_set_table_prism", "cd_get_table_prism", "cd_prism_struct_size", "cd_get_prism_stats", "cd_get_prism_hull", "cd_table_prism",
    "cd_prism_project", "cd_prism_hull_host",
    "cd_set_pair_score", "cd_get_pair_score", "cd_pair_score_struct_size", "cd_get_cluster_pair_scores", "cd_pair_score_points",
    "cd_pair_score_host",
    "cd_set_pose_info", "cd_get_pose_info", "cd_pose_info_struct_size", "cd_get_cluster_pose_info", "cd_pose_info_points", "cd_pose_info_host",
    "cd_pose_info_ros_covariance",
    "cd_set_box_fit", "cd_get_box_fit", "cd_box_fit_struct_size", "cd_get_cluster_box_fits", "cd_box_fit_points", "cd_box_fit_host", "cd_box_fit_match",
    "cd_set_box_select", "cd_get_box_select",
]

# rule C17 (cd_set_icp_plane_weight): the recommended setting and the least tangent weight
CD_ICP_PLANE_WEIGHT_DEFAULT, CD_ICP_PLANE_SWITCH_DEFAULT, CD_ICP_PLANE_WEIGHT_MIN = 1.0 / 32.0, 0.01, 1.0 / 1024.0

# rule C18 (cd_set_icp_coarse): the largest stride, and cd_icp_coarse_stats.used
CD_ICP_COARSE_STRIDE_MAX = 64
CD_COARSE_NOT_ELIGIBLE, CD_COARSE_USED, CD_COARSE_FELL_BACK = 0, 1, 2

CD_CLOUD_VOXELS, CD_CLOUD_OBJECTS = 0, 1
CD_GUESS_NONE, CD_GUESS_PARAMS, CD_GUESS_PER_FRAME, CD_GUESS_SURFACE, CD_GUESS_CLUSTER = 0, 1, 2, 3, 4


CD_PLANE, CD_PLANE_PERPENDICULAR, CD_PLANE_PARALLEL = 0, 1, 2
CD_COLOR_NONE, CD_COLOR_RGB8 = 0, 1
CD_BBOX_PARAMS, CD_BBOX_PER_FRAME, CD_BBOX_COLOR = 0, 1, 2
CD_DRAW_ACCEPTED, CD_DRAW_ALL = 0, 1
CD_VERIFY_ACCEPTED, CD_VERIFY_ALL = 0, 1
CD_VERIFY_MISS, CD_VERIFY_AGREE, CD_VERIFY_THROUGH, CD_VERIFY_OCCLUDED, CD_VERIFY_INVALID = 0, 1, 2, 3, 4
CD_NOTEX_DROP, CD_NOTEX_KEEP = 0, 1
CD_LABEL_INVALID, CD_LABEL_CROPPED, CD_LABEL_PLANE, CD_LABEL_OBJECT, CD_LABEL_GATED, CD_LABEL_CLUSTER0 = 0, 1, 2, 3, 4, 8
CD_OUTLIER_MAX_MEAN_K, CD_OUTLIER_LDS_TILE = 63, 1024
CD_PRISM_MAX_HULL, CD_PRISM_LDS_POINTS = 1024, 4096
# rule C21 (cd_set_pair_score): the recommended setting
CD_PAIR_SCORE_RANGE_DEFAULT, CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT, CD_PAIR_SCORE_MIN_INLIER_DEFAULT = 0.005, 0.5, 0.8
# rule C23 (cd_set_pose_info): the recommended setting
CD_POSE_INFO_RANGE_DEFAULT, CD_POSE_INFO_MIN_SUPPORT_DEFAULT = 0.005, 8.0
# rule C24 (cd_set_box_fit): the recommended band; the points of a cluster the kernel keeps in LDS
CD_BOX_FIT_BAND_DEFAULT, CD_BOX_FIT_LDS_POINTS = 0.006, 2048


class CdSurfaceFrameResult(C.Structure):
    _fields_ = [("Rt", C.c_float * 16), ("coeff", (C.c_float * 4) * 3), ("midpoint", (C.c_float * 4) * 3),
                ("n_points", C.c_int32 * 3), ("iterations", C.c_int32 * 3), ("reserved", C.c_int32 * 2)]


class CdIcpCoarseStats(C.Structure):
    """cd_icp_coarse_stats: what rule C18 did for one (cluster, template) pair."""
    _fields_ = [("n_coarse", C.c_int32), ("coarse_iterations", C.c_int32), ("coarse_converged", C.c_int32), ("coarse_status", C.c_int32),
                ("coarse_fitness", C.c_double), ("used", C.c_int32), ("reserved", C.c_int32)]


class CdIcpRejectStats(C.Structure):
    """cd_icp_reject_stats: what rule C19 did for one (cluster, template) pair."""
    _fields_ = [("first_kept", C.c_int32), ("last_kept", C.c_int32), ("min_kept", C.c_int32), ("stopped_few", C.c_int32),
                ("last_median", C.c_float), ("reserved", C.c_int32 * 3)]


class CdIcpRecipStats(C.Structure):
    """cd_icp_recip_stats: what rule C22 did for one (cluster, template) pair."""
    _fields_ = [("first_kept", C.c_int32), ("last_kept", C.c_int32), ("min_kept", C.c_int32), ("stopped_few", C.c_int32),
                ("last_n0", C.c_int32), ("reserved", C.c_int32 * 3)]


class CdPrismStats(C.Structure):
    """cd_prism_stats: what the table prism (rule C20) did to one cloud."""
    _fields_ = [("n_before", C.c_int32), ("n_kept", C.c_int32), ("n_below", C.c_int32), ("n_above", C.c_int32), ("n_outside", C.c_int32),
                ("hull_vertices", C.c_int32), ("axis_u", C.c_int32), ("axis_v", C.c_int32), ("overflow", C.c_int32), ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_[:9]}


class CdPairScore(C.Structure):
    """cd_pair_score: the two-way registration score (rule C21) of one (cluster, template) pair."""
    _fields_ = [("n_source", C.c_int32), ("n_source_in", C.c_int32), ("n_template", C.c_int32), ("n_template_in", C.c_int32), ("valid", C.c_int32),
                ("status", C.c_int32), ("forward_fitness_in", C.c_double), ("reverse_fitness_in", C.c_double), ("reverse_fitness", C.c_double),
                ("coverage", C.c_double), ("inlier_fraction", C.c_double)]

    def as_dict(self):
        return {k: (float if t is C.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class CdPoseInfo(C.Structure):
    """cd_pose_info: the pose information (rule C23) of one (cluster, lattice template) pair."""
    _fields_ = [("n_source", C.c_int32), ("n_in", C.c_int32), ("n_face", C.c_int32 * 3), ("n_constrained", C.c_int32), ("well_posed", C.c_int32),
                ("status", C.c_int32), ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36), ("weakest", C.c_double * 6),
                ("sigma2", C.c_double), ("covariance", C.c_double * 36), ("centre", C.c_double * 3), ("length", C.c_double)]

    def as_dict(self):
        """Scalars as int / float, arrays as lists."""
        out = {}
        for k, t in self._fields_:
            v = getattr(self, k)
            out[k] = list(v) if hasattr(v, "__len__") else (float(v) if t is C.c_double else int(v))
        return out


class CdBoxFit(C.Structure):
    """cd_box_fit: the box fit (rule C24) of one cluster - dims (L >= W, H), pose (row-major 4 x 4, box -> camera), the counts and its
    own status."""
    _fields_ = [("n", C.c_int32), ("n_top", C.c_int32), ("hull_vertices", C.c_int32), ("edge", C.c_int32), ("status", C.c_int32), ("overflow", C.c_int32),
                ("match_slot", C.c_int32), ("reserved", C.c_int32), ("height_ref", C.c_double), ("dims", C.c_double * 3), ("pose", C.c_double * 16),
                ("area", C.c_double), ("rectangularity", C.c_double), ("match_cost", C.c_double)]

    def as_dict(self):
        """Scalars as int / float, arrays as float64 arrays (the fields of perception_amd.box_fit's records)."""
        out = {}
        for k, t in self._fields_:
            v = getattr(self, k)
            out[k] = np.array(list(v), np.float64) if hasattr(v, "__len__") else (float(v) if t is C.c_double else int(v))
        return out


class CdShapeFrame(C.Structure):
    """cd_shape_frame: the principal frame of a point set (rule C13) - axes row-major with the axes as columns, variances
    descending, extents relative to the mean; status != CD_OK: n, status and zeros."""
    _fields_ = [("n", C.c_int32), ("status", C.c_int32), ("mean", C.c_double * 3), ("axes", C.c_double * 9),
                ("var", C.c_double * 3), ("lo", C.c_double * 3), ("hi", C.c_double * 3)]


class CdParams(C.Structure):
    _fields_ = [
        ("crop_z_min", C.c_double), ("crop_z_max", C.c_double),
        ("crop_x_min", C.c_double), ("crop_x_max", C.c_double),
        ("leaf_size", C.c_float), ("rgb_offset", C.c_int32),
        ("plane_distance_threshold", C.c_double),
        ("plane_max_iterations", C.c_int32), ("plane_optimize", C.c_int32),
        ("plane_probability", C.c_double),
        ("extract_negative", C.c_int32), ("crop2_enable", C.c_int32),
        ("crop2_z_min", C.c_double), ("crop2_z_max", C.c_double),
        ("cluster_enable", C.c_int32),
        ("cluster_min_size", C.c_int32), ("cluster_max_size", C.c_int32),
        ("cluster_tolerance", C.c_double),
        ("icp_max_iterations", C.c_int32), ("template_slot", C.c_int32),
        ("icp_transformation_epsilon", C.c_double),
        ("icp_euclidean_fitness_epsilon", C.c_double),
        ("icp_accept_fitness", C.c_double),
        ("bbox_P", C.c_double * 12), ("bbox_enable", C.c_int32), ("bbox_rect", C.c_int32 * 4),
        ("plane_model", C.c_int32), ("plane_axis", C.c_float * 3), ("plane_eps_angle", C.c_double),
        ("icp_use_guess", C.c_int32), ("icp_guess", C.c_float * 16),
    ]


class CdClusterResult(C.Structure):
    _fields_ = [
        ("size", C.c_int32), ("iterations", C.c_int32),
        ("converged", C.c_int32), ("accepted", C.c_int32),
        ("template_slot", C.c_int32), ("reserved", C.c_int32),
        ("T", C.c_float * 16), ("fitness", C.c_double), ("pose", C.c_double * 16),
    ]


class CdFrameResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("n_cropped", C.c_int32), ("n_voxels", C.c_int32),
        ("n_plane", C.c_int32), ("n_objects", C.c_int32), ("n_clusters", C.c_int32),
        ("ransac_iterations", C.c_int32), ("flags", C.c_int32),
        ("plane", C.c_float * 4), ("pad", C.c_float * 4),
        ("clusters", CdClusterResult * CD_MAX_CLUSTERS_PER_FRAME),
    ]


class CdTiming(C.Structure):
    _fields_ = [
        ("stage_ms", C.c_float * 5), ("icp_kernel_ms", C.c_float),
        ("icp_kernel_launches", C.c_int32),
        ("icp_pair_tests_lo", C.c_int32), ("icp_pair_tests_hi", C.c_int32), ("icp_persist_gave_up", C.c_int32),
        ("algorithmic_bytes", C.c_int64), ("icp_algorithmic_bytes", C.c_int64),
        ("scan_retries", C.c_int32), ("icp_regime", C.c_int32),
        ("icp_handovers", C.c_int32), ("icp_search", C.c_int32),
        ("icp_handover_lost", C.c_int32), ("icp_wave_ms", C.c_float),
    ]


class CdDepthCamera(C.Structure):
    """cd_depth_camera: CameraInfo of a 16UC1 depth stream (optionally with an rgb8 image registered to it)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("depth_scale", C.c_float), ("color", C.c_int32),
    ]


class CdColorCamera(C.Structure):
    """cd_color_camera: CameraInfo of the rgb8 colour stream of an UNREGISTERED pair, the depth -> colour extrinsics
    (p_colour = R p_depth + t, R row-major) and what becomes of a point that projects outside the colour image (rule C12)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("R", C.c_float * 9), ("t", C.c_float * 3),
        ("no_texture", C.c_int32), ("reserved", C.c_int32),
    ]


class CdColorGateParams(C.Structure):
    """cd_color_gate_params: the parameters of canonical rule C10 (the red-object rectangle of the colour branch)."""
    _fields_ = [("h_lo_max", C.c_int32), ("h_hi_min", C.c_int32), ("s_min", C.c_int32), ("v_min", C.c_int32),
                ("margin", C.c_int32), ("reserved", C.c_int32 * 3)]


class CdColorBBox(C.Structure):
    """cd_color_bbox: one frame's rectangle (x1, y1, x2, y2; all zero when found == 0) and what it was picked from."""
    _fields_ = [("rect", C.c_int32 * 4), ("found", C.c_int32), ("area2", C.c_int32), ("n_components", C.c_int32),
                ("n_mask", C.c_int32)]


class CdOverlayParams(C.Structure):
    """cd_overlay_params: the parameters of canonical rule C11 (the projected boxes of draw_bbox.py)."""
    _fields_ = [("P", C.c_double * 12), ("E", C.c_double * 16), ("dims", C.c_double * 3), ("thickness", C.c_int32),
                ("rgb", C.c_uint8 * 3), ("pad", C.c_uint8), ("reserved", C.c_int32 * 6)]


class CdOverlayBox(C.Structure):
    """cd_overlay_box: one box's projected corners u0, v0 .. u7, v7 (all zero when drawn == 0: skipped, or an empty slot)."""
    _fields_ = [("corners", C.c_int32 * 16), ("drawn", C.c_int32), ("reserved", C.c_int32 * 3)]


class CdVerifyParams(C.Structure):
    """cd_verify_params: the parameters of canonical rule C14 (an ICP pose's box rendered into the depth image)."""
    _fields_ = [("dims", C.c_double * 3), ("slot_dims", (C.c_double * 3) * CD_MAX_TEMPLATES), ("tolerance", C.c_double),
                ("min_score", C.c_double), ("min_agree", C.c_int32), ("use_slot_dims", C.c_int32), ("reserved", C.c_int32 * 6)]


class CdVerifyBox(C.Structure):
    """cd_verify_box: one box's pixel counts, their verdict and score (all zero for an empty slot or a box that was not rendered)."""
    _fields_ = [("verified", C.c_int32), ("passed", C.c_int32), ("n_hit", C.c_int32), ("n_agree", C.c_int32),
                ("n_through", C.c_int32), ("n_occluded", C.c_int32), ("n_invalid", C.c_int32), ("reserved", C.c_int32),
                ("agree_abs_um", C.c_int64), ("score", C.c_double)]


FRAME_RESULT_BYTES = C.sizeof(CdFrameResult)


class CdLabelPalette(C.Structure):
    _fields_ = [("rgba", (C.c_uint8 * 4) * 256)]


def default_label_palette():
    """The default palette of cd_tint_labels_batch as a (256, 4) uint8 array: r g b alpha per label."""
    p = CdLabelPalette()
    load_library().cd_default_label_palette(C.byref(p))
    return np.frombuffer(bytes(p), np.uint8).reshape(256, 4).copy()


def default_verify_params():
    """dims 0.2 / 0.1 / 0.03 (also in every slot_dims row), tolerance 0.01, min_score 0.9, min_agree 200.  Pure Python mirror of
    cd_default_verify_params()."""
    from . import verify
    p = CdVerifyParams()
    p.dims[:] = verify.DEFAULT_DIMS
    for row in p.slot_dims:
        row[:] = verify.DEFAULT_DIMS
    p.tolerance, p.min_score, p.min_agree = verify.DEFAULT_TOLERANCE, verify.DEFAULT_MIN_SCORE, verify.DEFAULT_MIN_AGREE
    return p


def verify_params(dims=None, slot_dims=None, tolerance=None, min_score=None, min_agree=None, use_slot_dims=None):
    """default_verify_params() with the given fields replaced (slot_dims: {slot: (l, w, h)} or a sequence of rows)."""
    p = default_verify_params()
    if dims is not None:
        p.dims[:] = [float(v) for v in dims]
    if slot_dims is not None:
        for k, row in (slot_dims.items() if isinstance(slot_dims, dict) else enumerate(slot_dims)):
            p.slot_dims[k][:] = [float(v) for v in row]
    if tolerance is not None:
        p.tolerance = float(tolerance)
    if min_score is not None:
        p.min_score = float(min_score)
    if min_agree is not None:
        p.min_agree = int(min_agree)
    if use_slot_dims is not None:
        p.use_slot_dims = int(use_slot_dims)
    return p


def default_overlay_params():
    """D435 P (the K of default_depth_camera, zero fourth column), E = identity, dims 0.2 / 0.1 / 0.03, thickness 2, green.
    Pure Python mirror of cd_default_overlay_params()."""
    from . import overlay
    o = CdOverlayParams()
    o.P[:] = overlay.DEFAULT_P
    o.E[:] = overlay.DEFAULT_E
    o.dims[:] = overlay.DEFAULT_DIMS
    o.thickness = overlay.DEFAULT_THICKNESS
    o.rgb[:] = overlay.DEFAULT_RGB
    return o


def overlay_params(P=None, E=None, dims=None, thickness=None, rgb=None):
    """default_overlay_params() with the given fields replaced (P 3x4, E 4x4, dims l / w / h, thickness, rgb)."""
    o = default_overlay_params()
    if P is not None:
        o.P[:] = [float(v) for v in np.asarray(P, np.float64).reshape(12)]
    if E is not None:
        o.E[:] = [float(v) for v in np.asarray(E, np.float64).reshape(16)]
    if dims is not None:
        o.dims[:] = [float(v) for v in dims]
    if thickness is not None:
        o.thickness = int(thickness)
    if rgb is not None:
        o.rgb[:] = [int(v) for v in rgb]
    return o


def default_color_gate_params():
    """object_detection.py's constants: H 0..10 or 175..179, S >= 50, V >= 100, margin 10.  Pure Python mirror of
    cd_default_color_gate_params()."""
    g = CdColorGateParams()
    g.h_lo_max, g.h_hi_min, g.s_min, g.v_min, g.margin = 10, 175, 50, 100, 10
    return g


def default_params():
    """cuboid_detection launch values (ground_plane_segmentation.launch:14-18,
    iterative_closest_point.launch:39-42) + object_detection's cluster constants
    (object_pose_detection.cpp:356-358).  Pure Python mirror of cd_default_params()."""
    p = CdParams()
    p.crop_z_min, p.crop_z_max = 0.0, 0.9
    p.crop_x_min, p.crop_x_max = -0.2, 0.2
    p.leaf_size = 0.005
    p.rgb_offset = -1
    p.plane_distance_threshold = 0.015
    p.plane_max_iterations = 1000
    p.plane_optimize = 1
    p.plane_probability = 0.99
    p.extract_negative = 1
    p.crop2_enable = 1
    p.crop2_z_min, p.crop2_z_max = 0.0, 0.75
    p.cluster_enable = 1
    p.cluster_min_size, p.cluster_max_size = 200, 25000
    p.cluster_tolerance = 0.02
    p.icp_max_iterations = 5000
    p.template_slot = 0
    p.icp_transformation_epsilon = 1e-9
    p.icp_euclidean_fitness_epsilon = 0.0004
    p.icp_accept_fitness = 0.0004
    return p


def default_depth_camera():
    """The D435 depth stream of the reference's README.md:74-78 (640 x 480, K of its CameraInfo), 1 mm per unit, no
    colour.  Pure Python mirror of cd_default_depth_camera()."""
    cam = CdDepthCamera()
    cam.width, cam.height = 640, 480
    cam.fx = cam.fy = 384.0898742675781
    cam.cx, cam.cy = 322.4656677246094, 240.64073181152344
    cam.depth_scale = 0.001
    cam.color = CD_COLOR_NONE
    return cam


def default_color_camera():
    """The D435 colour stream of the reference's README.md:48-54 (640 x 480, K of its CameraInfo), R = identity, t = 0 (the
    reference records no extrinsic values), CD_NOTEX_DROP.  Pure Python mirror of cd_default_color_camera()."""
    cc = CdColorCamera()
    cc.width, cc.height = 640, 480
    cc.fx, cc.fy = 616.8246459960938, 616.609375
    cc.cx, cc.cy = 321.81976318359375, 239.91116333007812
    cc.R[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    cc.no_texture = CD_NOTEX_DROP
    return cc


def color_camera(width=None, height=None, K=None, R=None, t=None, no_texture=None):
    """default_color_camera() with the given fields replaced (K = fx, fy, cx, cy; R 3x3 row-major depth -> colour; t metres)."""
    cc = default_color_camera()
    if width is not None:
        cc.width = int(width)
    if height is not None:
        cc.height = int(height)
    if K is not None:
        cc.fx, cc.fy, cc.cx, cc.cy = (float(v) for v in K)
    if R is not None:
        cc.R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    if t is not None:
        cc.t[:] = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
    if no_texture is not None:
        cc.no_texture = int(no_texture)
    return cc


_lib = None


def load_library(path=None):
    """dlopen libcuboid_hip.so and set prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            "libcuboid_hip.so not found at %s: the HIP extension is not built and there is "
            "no CPU fallback (build with `make -C perception_amd/csrc`)" % p)
    lib = C.CDLL(p)
    vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ip = C.POINTER(C.c_int)
    lib.cd_default_params.argtypes = [C.POINTER(CdParams)]
    lib.cd_default_params.restype = None
    lib.cd_abi_version.restype = C.c_int
    lib.cd_struct_size.argtypes = [C.c_int]
    lib.cd_struct_size.restype = C.c_int
    lib.cd_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.cd_destroy.argtypes = [vp]
    lib.cd_destroy.restype = None
    lib.cd_last_error.argtypes = [vp]
    lib.cd_last_error.restype = C.c_char_p
    lib.cd_set_template.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int]
    lib.cd_crop_voxel.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(CdParams), vp, vp,
                                  C.c_int, ip, ip]
    lib.cd_segment_plane.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(CdParams), vp, vp,
                                     C.c_int, ip, ip]
    lib.cd_surface_frame.argtypes = [vp, vp, C.c_size_t, C.c_int, f32p, C.c_int, C.POINTER(CdParams), C.POINTER(CdSurfaceFrameResult)]
    lib.cd_bbox_filter.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, vp, vp, C.c_int, ip]
    lib.cd_extract.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, ip]
    lib.cd_cluster.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(CdParams), vp, vp, C.c_int, ip]
    lib.cd_icp.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, C.POINTER(CdParams),
                           C.POINTER(CdClusterResult), vp]
    for f in (lib.cd_process_batch, lib.cd_process_batch_device):
        f.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(CdParams), vp, vp, vp]
    lib.cd_process_frame.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(CdParams), vp, vp, vp]
    lib.cd_get_cluster_results.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(CdClusterResult), ip]
    lib.cd_pose_to_position_quaternion.argtypes = [C.POINTER(C.c_double)] * 3
    lib.cd_pose_to_position_quaternion.restype = None
    lib.cd_bbox_corners.argtypes = [C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, f32p]
    lib.cd_bbox_corners.restype = None
    lib.cd_get_timing.argtypes = [vp, C.POINTER(CdTiming)]
    lib.cd_get_frame_cloud.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, ip]
    lib.cd_get_cluster_points.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, ip]
    lib.cd_ground_plane.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(CdParams), f32p, vp, C.c_int, ip, ip]
    lib.cd_set_frame_guesses.argtypes = [vp, f32p, C.c_int]
    lib.cd_surface_batch.argtypes = [vp, vp, C.c_size_t, C.c_int, i32p, C.c_int, f32p, C.c_int, C.POINTER(CdParams),
                                     C.POINTER(CdSurfaceFrameResult), i32p]
    lib.cd_surface_guess.argtypes = [f32p, f32p]
    lib.cd_set_surface_distance_threshold.argtypes = [vp, C.c_double]
    lib.cd_get_surface_distance_threshold.argtypes = [vp, C.POINTER(C.c_double)]
    lib.cd_get_surface_results.argtypes = [vp, C.c_int, C.c_int, C.POINTER(CdSurfaceFrameResult), i32p]
    lib.cd_template_lattice_faces.argtypes = [vp, C.c_int]
    lib.cd_template_nearest.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, vp, vp]
    lib.cd_icp_solve_batch.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, vp, vp, vp, vp]
    lib.cd_lattice_detect.argtypes = [vp, C.c_size_t, C.c_int, vp]
    lib.cd_lattice_axes.argtypes = [vp, C.c_size_t, C.c_int, vp, vp]
    lib.cd_set_icp_max_correspondence_distance.argtypes = [vp, C.c_double]
    lib.cd_get_icp_max_correspondence_distance.argtypes = [vp, C.POINTER(C.c_double)]
    lib.cd_icp_correspondence_threshold.argtypes = [C.c_double, C.POINTER(C.c_float), ip]
    lib.cd_passthrough.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, vp, C.c_int, ip]
    lib.cd_default_depth_camera.argtypes = [C.POINTER(CdDepthCamera)]
    lib.cd_default_depth_camera.restype = None
    lib.cd_depth_to_cloud.argtypes = [vp, C.POINTER(CdDepthCamera), vp, vp, vp, C.c_size_t, C.c_int, C.c_int, ip]
    for f in (lib.cd_process_depth_batch, lib.cd_process_depth_batch_device):
        f.argtypes = [vp, C.POINTER(CdDepthCamera), vp, vp, C.c_int, C.POINTER(CdParams), vp, vp, vp]
    lib.cd_default_color_gate_params.argtypes = [C.POINTER(CdColorGateParams)]
    lib.cd_default_color_gate_params.restype = None
    for f in (lib.cd_color_bbox_batch, lib.cd_color_bbox_batch_device):
        f.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(CdColorGateParams), C.POINTER(CdColorBBox)]
    lib.cd_set_frame_bboxes.argtypes = [vp, i32p, C.c_int]
    lib.cd_set_bbox_source.argtypes = [vp, C.c_int, C.POINTER(CdColorGateParams)]
    lib.cd_get_bbox_source.argtypes = [vp, ip]
    lib.cd_get_frame_bboxes.argtypes = [vp, C.c_int, C.c_int, C.POINTER(CdColorBBox)]
    dp = C.POINTER(C.c_double)
    lib.cd_default_overlay_params.argtypes = [C.POINTER(CdOverlayParams)]
    lib.cd_default_overlay_params.restype = None
    lib.cd_overlay_project.argtypes = [dp, C.POINTER(CdOverlayParams), C.POINTER(CdOverlayBox)]
    for f in (lib.cd_draw_boxes_batch, lib.cd_draw_boxes_batch_device):
        f.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, dp, i32p, C.c_int, C.POINTER(CdOverlayParams), C.POINTER(CdOverlayBox)]
    for f in (lib.cd_draw_last_results, lib.cd_draw_last_results_device):
        f.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(CdOverlayParams), C.POINTER(CdOverlayBox)]
    vpp, vbp, dcp = C.POINTER(CdVerifyParams), C.POINTER(CdVerifyBox), C.POINTER(CdDepthCamera)
    lib.cd_default_verify_params.argtypes = [vpp]
    lib.cd_default_verify_params.restype = None
    lib.cd_verify_struct_size.argtypes = [C.c_int]
    lib.cd_verify_pixel.argtypes = [dcp, dp, vpp, C.c_int, C.c_int, C.c_uint16, i32p, dp]
    lib.cd_verify_box_host.argtypes = [dcp, vp, dp, vpp, vbp]
    for f in (lib.cd_verify_boxes_batch, lib.cd_verify_boxes_batch_device):
        f.argtypes = [vp, dcp, vp, C.c_int, dp, i32p, C.c_int, dp, vpp, vbp]
    for f in (lib.cd_verify_last_results, lib.cd_verify_last_results_device):
        f.argtypes = [vp, dcp, vp, C.c_int, vpp, vbp]
    lib.cd_default_color_camera.argtypes = [C.POINTER(CdColorCamera)]
    lib.cd_default_color_camera.restype = None
    lib.cd_color_camera_struct_size.argtypes = []
    lib.cd_texture_project.argtypes = [C.POINTER(CdDepthCamera), C.POINTER(CdColorCamera), C.c_int, C.c_int, C.c_uint16, f32p, i32p, i32p]
    lib.cd_depth_to_cloud_mapped.argtypes = [vp, C.POINTER(CdDepthCamera), C.POINTER(CdColorCamera), vp, vp, vp, C.c_size_t, C.c_int,
                                             C.c_int, ip]
    for f in (lib.cd_process_depth_batch_mapped, lib.cd_process_depth_batch_mapped_device):
        f.argtypes = [vp, C.POINTER(CdDepthCamera), C.POINTER(CdColorCamera), vp, vp, C.c_int, C.POINTER(CdParams), vp, vp, vp]
    sfp = C.POINTER(CdShapeFrame)
    lib.cd_shape_frame_struct_size.argtypes = []
    lib.cd_shape_frame_host.argtypes = [vp, C.c_size_t, C.c_int, sfp]
    lib.cd_shape_frames.argtypes = [vp, vp, C.c_size_t, i32p, C.c_int, sfp]
    lib.cd_template_shape_frame.argtypes = [vp, C.c_int, sfp]
    lib.cd_shape_guess.argtypes = [sfp, sfp, f32p, i32p]
    lib.cd_get_cluster_shape_frames.argtypes = [vp, C.c_int, C.c_int, C.c_int, sfp]
    lpp, u8p = C.POINTER(CdLabelPalette), C.c_void_p
    for f in (lib.cd_label_points_last, lib.cd_label_points_last_device):
        f.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, u8p]
    for f in (lib.cd_label_depth_last, lib.cd_label_depth_last_device):
        f.argtypes = [vp, dcp, vp, C.c_int, u8p]
    lib.cd_default_label_palette.argtypes = [lpp]
    lib.cd_default_label_palette.restype = None
    lib.cd_label_struct_size.argtypes = [C.c_int]
    for f in (lib.cd_tint_labels_batch, lib.cd_tint_labels_batch_device):
        f.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_int, lpp]
    lib.cd_set_outlier_filter.argtypes = [vp, C.c_int, C.c_double, C.c_int]
    lib.cd_get_outlier_filter.argtypes = [vp, ip, dp, ip]
    lib.cd_get_outlier_stats.argtypes = [vp, C.c_int, ip, ip, dp, dp, dp]
    lib.cd_outlier_filter.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_int, vp, C.c_int, ip, vp, vp]
    lib.cd_set_icp_plane_weight.argtypes = [vp, C.c_double, C.c_double]
    lib.cd_get_icp_plane_weight.argtypes = [vp, dp, dp]
    lib.cd_get_cluster_plane_stats.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.cd_icp_plane_solve_host.argtypes = [vp, C.c_int, vp, ip]
    lib.cd_set_icp_coarse.argtypes = [vp, C.c_int, C.c_int]
    lib.cd_get_icp_coarse.argtypes = [vp, ip, ip]
    lib.cd_icp_coarse_struct_size.argtypes = []
    lib.cd_icp_coarse_subsample.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int]
    lib.cd_get_cluster_coarse_stats.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.cd_set_icp_median_rejection.argtypes = [vp, C.c_double]
    lib.cd_get_icp_median_rejection.argtypes = [vp, dp]
    lib.cd_icp_reject_struct_size.argtypes = []
    lib.cd_get_cluster_reject_stats.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.cd_icp_median_threshold.argtypes = [vp, C.c_int, C.c_double, vp, dp]
    lib.cd_set_icp_reciprocal.argtypes = [vp, C.c_int]
    lib.cd_get_icp_reciprocal.argtypes = [vp, ip]
    lib.cd_icp_recip_struct_size.argtypes = []
    lib.cd_get_cluster_recip_stats.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.cd_icp_reciprocal_mask.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int, C.c_float, vp, vp, vp]
    psp = C.POINTER(CdPrismStats)
    lib.cd_set_table_prism.argtypes = [vp, C.c_int, C.c_double, C.c_double]
    lib.cd_get_table_prism.argtypes = [vp, ip, dp, dp]
    lib.cd_prism_struct_size.argtypes = []
    lib.cd_get_prism_stats.argtypes = [vp, C.c_int, psp]
    lib.cd_get_prism_hull.argtypes = [vp, C.c_int, vp, C.c_int, ip]
    lib.cd_table_prism.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, vp, C.c_size_t, C.c_int, C.c_double, C.c_double, vp, C.c_int, ip, psp, vp, C.c_int]
    lib.cd_prism_project.argtypes = [vp, vp, dp, vp, vp]
    lib.cd_prism_hull_host.argtypes = [vp, C.c_int, vp, C.c_int, ip]
    pcp = C.POINTER(CdPairScore)
    lib.cd_set_pair_score.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.cd_get_pair_score.argtypes = [vp, ip, dp, dp, dp]
    lib.cd_pair_score_struct_size.argtypes = []
    lib.cd_get_cluster_pair_scores.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.cd_pair_score_points.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, vp, C.c_double, C.c_double, C.c_double, C.c_int, pcp]
    lib.cd_pair_score_host.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int, vp, C.c_double, C.c_double, C.c_double, C.c_int, pcp]
    pip = C.POINTER(CdPoseInfo)
    lib.cd_set_pose_info.argtypes = [vp, C.c_int, C.c_double, C.c_double]
    lib.cd_get_pose_info.argtypes = [vp, ip, dp, dp]
    lib.cd_pose_info_struct_size.argtypes = []
    lib.cd_get_cluster_pose_info.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.cd_pose_info_points.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, vp, C.c_double, C.c_double, C.c_int, pip]
    lib.cd_pose_info_host.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int, vp, C.c_double, C.c_double, C.c_int, pip]
    lib.cd_pose_info_ros_covariance.argtypes = [pip, vp, vp]
    bfp = C.POINTER(CdBoxFit)
    lib.cd_set_box_fit.argtypes = [vp, C.c_int, C.c_double]
    lib.cd_get_box_fit.argtypes = [vp, ip, dp]
    lib.cd_box_fit_struct_size.argtypes = []
    lib.cd_get_cluster_box_fits.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.cd_box_fit_points.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_int32), C.c_int, C.c_double, vp]
    lib.cd_box_fit_host.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_double, bfp]
    lib.cd_set_box_select.argtypes = [vp, C.c_int, vp, C.c_double]
    lib.cd_get_box_select.argtypes = [vp, ip, vp, dp]
    lib.cd_box_fit_match.argtypes = [vp, vp, C.c_uint32, C.c_double, C.POINTER(C.c_int32), dp]
    if path is None:
        _lib = lib
    return lib


class CuboidError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("cd status %d: %s" % (status, msg))
        self.status = status


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _points(a):
    """(base pointer, stride, n) of a 2-D float32 array whose rows start with x,y,z."""
    a = np.ascontiguousarray(a, dtype=np.float32) if a.dtype != np.float32 or not a.flags.c_contiguous else a
    assert a.ndim == 2 and a.shape[1] >= 3
    return a, (a.strides[0] if a.shape[0] else 4 * a.shape[1]), a.shape[0]   # numpy reports stride 0 for empty arrays


class Context:
    """One GPU context (cd_create/cd_destroy).  Not thread-safe, like the reference node."""

    def __init__(self, max_points, max_frames=1, device_id=0):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.cd_create(device_id, int(max_points), int(max_frames), C.byref(h))
        if st != CD_OK:
            raise CuboidError(st, "cd_create failed (no usable HIP device? there is no CPU fallback)")
        self.h = h
        self.max_points, self.max_frames = int(max_points), int(max_frames)

    def close(self):
        if getattr(self, "h", None):
            self.lib.cd_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, st, ok=(CD_OK,)):
        if st not in ok:
            raise CuboidError(st, (self.lib.cd_last_error(self.h) or b"").decode())
        return st

    def set_template(self, slot, xyz):
        a, stride, m = _points(xyz)
        self._check(self.lib.cd_set_template(self.h, slot, _ptr(a), stride, m))

    def crop_voxel(self, points, prm, want_rgb=False):
        a, stride, n = _points(points)
        out = np.empty((n, 3), np.float32)
        rgb = np.empty(n, np.uint32) if want_rgb else None
        nc, nv = C.c_int(), C.c_int()
        self._check(self.lib.cd_crop_voxel(self.h, _ptr(a), stride, n, C.byref(prm), _ptr(out), _ptr(rgb),
                                           n, C.byref(nc), C.byref(nv)))
        return out[:nv.value].copy(), (rgb[:nv.value].copy() if want_rgb else None), nc.value

    def segment_plane(self, xyz, prm):
        a, stride, n = _points(xyz)
        coeff = np.zeros(4, np.float32)
        inl = np.empty(max(n, 1), np.int32)
        ni, it = C.c_int(), C.c_int()
        st = self.lib.cd_segment_plane(self.h, _ptr(a), stride, n, C.byref(prm), _ptr(coeff), _ptr(inl), n,
                                       C.byref(ni), C.byref(it))
        self._check(st, ok=(CD_OK, CD_ERR_NO_MODEL))
        return st, coeff, inl[:ni.value].copy(), it.value

    def cluster(self, xyz, prm, sizes_capacity=4096):
        a, stride, n = _points(xyz)
        labels = np.empty(max(n, 1), np.int32)
        sizes = np.zeros(sizes_capacity, np.int32)
        k = C.c_int()
        self._check(self.lib.cd_cluster(self.h, _ptr(a), stride, n, C.byref(prm), _ptr(labels), _ptr(sizes),
                                        sizes_capacity, C.byref(k)))
        return labels[:n].copy(), sizes[:min(k.value, sizes_capacity)].copy(), k.value

    def surface_frame(self, xyz, table_normal, prm, invert=True):
        """surface_normal_estimation.cpp's callback: three axis-constrained plane fits -> pose of the cuboid frame."""
        a, stride, n = _points(xyz)
        tn = np.ascontiguousarray(table_normal, np.float32)
        res = CdSurfaceFrameResult()
        st = self.lib.cd_surface_frame(self.h, _ptr(a), stride, n, tn.ctypes.data_as(C.POINTER(C.c_float)), 1 if invert else 0,
                                       C.byref(prm), C.byref(res))
        self._check(st, ok=(CD_OK, CD_ERR_NO_MODEL))
        return st, res

    def bbox_filter(self, xyz, P, rect):
        """bbox_filter.cpp: ascending indices of the points projecting strictly inside the rectangle."""
        a, stride, n = _points(xyz)
        Pm = np.ascontiguousarray(P, np.float64).ravel()
        r = np.ascontiguousarray(rect, np.int32)
        idx = np.empty(max(n, 1), np.int32)
        cnt = C.c_int()
        self._check(self.lib.cd_bbox_filter(self.h, _ptr(a), stride, n, _ptr(Pm), _ptr(r), _ptr(idx), max(n, 1), C.byref(cnt)))
        return idx[:cnt.value].copy()

    def icp(self, slot, src, prm, want_aligned=False):
        a, stride, n = _points(src)
        res = CdClusterResult()
        al = np.empty((n, 3), np.float32) if want_aligned else None
        st = self.lib.cd_icp(self.h, slot, _ptr(a), stride, n, C.byref(prm), C.byref(res), _ptr(al))
        self._check(st, ok=(CD_OK, CD_ERR_FEW_CORRESPONDENCES))
        return st, res, al

    def process_batch(self, frames, prm, want_indices=False):
        """frames: (F, N, C>=3) float32 host array.  Returns (results, plane_inliers, labels)."""
        f = np.ascontiguousarray(frames, dtype=np.float32)
        assert f.ndim == 3
        F, N, Cc = f.shape
        res = (CdFrameResult * F)()
        pi = np.empty((F, N), np.int32) if want_indices else None
        lb = np.empty((F, N), np.int32) if want_indices else None
        self._check(self.lib.cd_process_batch(self.h, _ptr(f), Cc * 4, N, F, C.byref(prm),
                                              C.cast(res, C.c_void_p), _ptr(pi), _ptr(lb)))
        return res, pi, lb

    def extract(self, records, indices, negative=True):
        """pcl::ExtractIndices on whole records: `records` is an (n, k) array of 4-byte items (all fields of a point)."""
        r = np.ascontiguousarray(records)
        assert r.ndim == 2 and r.dtype.itemsize == 4
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        n, stride = r.shape[0], r.shape[1] * 4
        out = np.empty((n if negative else len(idx), r.shape[1]), r.dtype)
        cnt = C.c_int()
        self._check(self.lib.cd_extract(self.h, _ptr(r), stride, n, _ptr(idx), len(idx), 1 if negative else 0, _ptr(out), len(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def process_frame(self, points, prm, want_indices=False):
        """One frame (N, C>=3) float32: the reference's callback body as one call.  Returns (result, plane_inliers, labels)."""
        f = np.ascontiguousarray(points, dtype=np.float32)
        assert f.ndim == 2
        N, Cc = f.shape
        res = CdFrameResult()
        pi = np.empty(N, np.int32) if want_indices else None
        lb = np.empty(N, np.int32) if want_indices else None
        self._check(self.lib.cd_process_frame(self.h, _ptr(f), Cc * 4, N, C.byref(prm), C.byref(res), _ptr(pi), _ptr(lb)))
        return res, pi, lb

    def process_batch_device(self, dev_ptr, stride_bytes, points_per_frame, n_frames, prm,
                             results=None, plane_inliers=None, labels=None):
        """Input already in HBM (e.g. a torch tensor's data_ptr())."""
        res = results if results is not None else (CdFrameResult * n_frames)()
        self._check(self.lib.cd_process_batch_device(self.h, C.c_void_p(dev_ptr), stride_bytes,
                                                     points_per_frame, n_frames, C.byref(prm),
                                                     C.cast(res, C.c_void_p), _ptr(plane_inliers),
                                                     _ptr(labels)))
        return res

    def process_batch_host_ptr(self, host_ptr, stride_bytes, points_per_frame, n_frames, prm, results=None):
        """cd_process_batch on a raw HOST pointer (e.g. a pinned torch tensor's data_ptr()): the upload is part of the call."""
        res = results if results is not None else (CdFrameResult * n_frames)()
        self._check(self.lib.cd_process_batch(self.h, C.c_void_p(host_ptr), stride_bytes, points_per_frame, n_frames,
                                              C.byref(prm), C.cast(res, C.c_void_p), None, None))
        return res

    def cluster_results(self, frame, first=0, count=None):
        """ICP results of EVERY cluster of `frame` of the last process_batch* call (opd.cpp:376 registers all of them; the
        fixed-size record holds the CD_MAX_CLUSTERS_PER_FRAME largest)."""
        tot = C.c_int()
        self._check(min(0, self.lib.cd_get_cluster_results(self.h, frame, 0, 0, None, C.byref(tot))))
        n = max(0, tot.value - first) if count is None else count
        out = (CdClusterResult * max(n, 1))()
        got = self.lib.cd_get_cluster_results(self.h, frame, first, n, out, None)
        self._check(min(0, got))
        return [out[i] for i in range(got)]

    def frame_cloud(self, frame, which, stride_bytes=16, rgb_offset=12):
        """Voxel cloud (CD_CLOUD_VOXELS) or object cloud (CD_CLOUD_OBJECTS) of `frame` of the last process_batch* call, as
        (n, stride_bytes / 4) uint32 records: x,y,z at words 0..2, packed rgb at rgb_offset (-1: none), the rest zero."""
        n = C.c_int()
        st = self.lib.cd_get_frame_cloud(self.h, frame, which, None, stride_bytes, rgb_offset, 0, C.byref(n))
        if st not in (CD_OK, CD_ERR_CAPACITY):
            self._check(st)
        out = np.zeros((max(n.value, 1), stride_bytes // 4), np.uint32)
        self._check(self.lib.cd_get_frame_cloud(self.h, frame, which, _ptr(out), stride_bytes, rgb_offset, n.value, C.byref(n)))
        return out[:n.value]

    def cluster_points(self, frame, k, aligned=False, stride_bytes=16):
        """Points of cluster k of `frame` of the last process_batch* call (aligned: the cloud icp.align returned), as
        (n, stride_bytes / 4) float32 records (fourth word 1.0f: pcl::PointXYZ's wire layout)."""
        n = C.c_int()
        st = self.lib.cd_get_cluster_points(self.h, frame, k, 1 if aligned else 0, None, stride_bytes, 0, C.byref(n))
        if st not in (CD_OK, CD_ERR_CAPACITY):
            self._check(st)
        out = np.zeros((max(n.value, 1), stride_bytes // 4), np.float32)
        self._check(self.lib.cd_get_cluster_points(self.h, frame, k, 1 if aligned else 0, _ptr(out), stride_bytes, n.value, C.byref(n)))
        return out[:n.value]

    def ground_plane(self, points, prm):
        """gps.cpp:43-112 as one call.  points: (n, k) float32 records.  Returns (status, coeff, kept records (m, k) uint32 view
        of the input's layout, n_inliers)."""
        a = np.ascontiguousarray(points, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] >= 3
        n, stride = a.shape[0], a.shape[1] * 4
        coeff = np.zeros(4, np.float32)
        out = np.zeros((max(n, 1), a.shape[1]), np.uint32)
        m, ni = C.c_int(), C.c_int()
        st = self.lib.cd_ground_plane(self.h, _ptr(a), stride, n, C.byref(prm), coeff.ctypes.data_as(C.POINTER(C.c_float)), _ptr(out), n,
                                      C.byref(m), C.byref(ni))
        self._check(st, ok=(CD_OK, CD_ERR_NO_MODEL))
        return st, coeff, out[:m.value].copy(), ni.value

    def set_frame_guesses(self, guesses):
        """Per-frame initial guesses (F, 4, 4) float32 for prm.icp_use_guess = CD_GUESS_PER_FRAME; None clears."""
        if guesses is None:
            self._check(self.lib.cd_set_frame_guesses(self.h, None, 0))
            return
        g = np.ascontiguousarray(guesses, np.float32).reshape(-1, 16)
        self._check(self.lib.cd_set_frame_guesses(self.h, g.ctypes.data_as(C.POINTER(C.c_float)), g.shape[0]))

    def color_bbox_batch(self, rgb, params=None):
        """Rule C10 on rgb (F, H, W, 3) uint8 host images: an array of F CdColorBBox (cd_color_bbox_batch)."""
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        assert a.ndim == 4 and a.shape[3] == 3
        F, H, W = a.shape[:3]
        out = (CdColorBBox * max(F, 1))()
        self._check(self.lib.cd_color_bbox_batch(self.h, _ptr(a), W, H, F, None if params is None else C.byref(params), out))
        return out

    def color_bbox_batch_device(self, rgb, params=None):
        """Same on a contiguous torch uint8 tensor (F, H, W, 3) in HBM (the caller has synchronised the stream that wrote it)."""
        assert rgb.is_contiguous() and rgb.dim() == 4 and rgb.shape[3] == 3
        F, H, W = (int(v) for v in rgb.shape[:3])
        out = (CdColorBBox * max(F, 1))()
        self._check(self.lib.cd_color_bbox_batch_device(self.h, C.c_void_p(rgb.data_ptr()), W, H, F,
                                                        None if params is None else C.byref(params), out))
        return out

    def set_frame_bboxes(self, rects):
        """Per-frame gate rectangles (F, 4) int32 (x1, y1, x2, y2) for the source CD_BBOX_PER_FRAME; None clears."""
        if rects is None:
            self._check(self.lib.cd_set_frame_bboxes(self.h, None, 0))
            return
        r = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
        self._check(self.lib.cd_set_frame_bboxes(self.h, r.ctypes.data_as(C.POINTER(C.c_int32)), r.shape[0]))

    def set_bbox_source(self, source, params=None):
        """Where the fused calls' gate (prm.bbox_enable) takes its rectangle from: CD_BBOX_PARAMS / _PER_FRAME / _COLOR."""
        self._check(self.lib.cd_set_bbox_source(self.h, source, None if params is None else C.byref(params)))

    def bbox_source(self):
        v = C.c_int()
        self._check(self.lib.cd_get_bbox_source(self.h, C.byref(v)))
        return v.value

    def frame_bboxes(self, first=0, count=None):
        """The rectangles the gate of the last fused call used (sources CD_BBOX_PER_FRAME / CD_BBOX_COLOR): a list of CdColorBBox."""
        cap = self.max_frames if count is None else count
        out = (CdColorBBox * max(cap, 1))()
        n = self.lib.cd_get_frame_bboxes(self.h, first, cap, out)
        if n < 0:
            raise CuboidError(n, "cd_get_frame_bboxes: the last fused call's gate did not read per-frame rectangles")
        return [out[i] for i in range(n)]

    def draw_boxes(self, rgb, poses, n_boxes=None, params=None):
        """Rule C11: the projected boxes of draw_bbox.py drawn IN PLACE into rgb, either a C-contiguous writable (F, H, W, 3)
        uint8 numpy array (cd_draw_boxes_batch: uploaded, drawn, downloaded) or a contiguous torch uint8 tensor of that shape in
        HBM (cd_draw_boxes_batch_device; the caller has synchronised the stream that wrote it).  poses (F, B, 4, 4) float64,
        n_boxes (F,) (None: all B).  Returns an array of F * B CdOverlayBox, box b of frame f at [f * B + b]."""
        on_device = not isinstance(rgb, np.ndarray)
        if on_device:
            assert rgb.is_contiguous() and rgb.dim() == 4 and rgb.shape[3] == 3
            ptr = C.c_void_p(rgb.data_ptr())
        else:
            assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3 and rgb.flags.c_contiguous and rgb.flags.writeable
            ptr = _ptr(rgb)
        F, H, W = (int(v) for v in rgb.shape[:3])
        p = np.ascontiguousarray(poses, np.float64).reshape(F, -1, 16)
        B = p.shape[1]
        nb = np.full(F, B, np.int32) if n_boxes is None else np.ascontiguousarray(n_boxes, np.int32)
        assert nb.shape == (F,)
        out = (CdOverlayBox * max(F * B, 1))()
        fn = self.lib.cd_draw_boxes_batch_device if on_device else self.lib.cd_draw_boxes_batch
        self._check(fn(self.h, ptr, W, H, F, p.ctypes.data_as(C.POINTER(C.c_double)), nb.ctypes.data_as(C.POINTER(C.c_int32)), B,
                       None if params is None else C.byref(params), out))
        return out

    def draw_last_results(self, rgb, which=CD_DRAW_ACCEPTED, params=None):
        """The poses of the last fused call drawn IN PLACE into its frames' images (numpy array or torch tensor as for
        draw_boxes; F = that call's frames).  which: CD_DRAW_ACCEPTED / CD_DRAW_ALL.  Returns F * CD_MAX_CLUSTERS_PER_FRAME
        CdOverlayBox, slot k of frame f = clusters[k] of its record.  Leaves the fused call's read-backs as they are."""
        on_device = not isinstance(rgb, np.ndarray)
        if on_device:
            assert rgb.is_contiguous() and rgb.dim() == 4 and rgb.shape[3] == 3
            ptr = C.c_void_p(rgb.data_ptr())
        else:
            assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3 and rgb.flags.c_contiguous and rgb.flags.writeable
            ptr = _ptr(rgb)
        F, H, W = (int(v) for v in rgb.shape[:3])
        out = (CdOverlayBox * (max(F, 1) * CD_MAX_CLUSTERS_PER_FRAME))()
        fn = self.lib.cd_draw_last_results_device if on_device else self.lib.cd_draw_last_results
        self._check(fn(self.h, ptr, W, H, int(which), None if params is None else C.byref(params), out))
        return out

    @staticmethod
    def _depth_images(depth):
        """(pointer, on_device, F, H, W) of a C-contiguous (F, H, W) uint16 numpy array or a contiguous 16-bit torch tensor in HBM."""
        on_device = not isinstance(depth, np.ndarray)
        if on_device:
            assert depth.is_contiguous() and depth.dim() == 3 and depth.element_size() == 2
            ptr = C.c_void_p(depth.data_ptr())
        else:
            assert depth.dtype == np.uint16 and depth.ndim == 3 and depth.flags.c_contiguous
            ptr = _ptr(depth)
        F, H, W = (int(v) for v in depth.shape)
        return ptr, on_device, F, H, W

    def verify_boxes(self, depth, poses, n_boxes, cam, params=None, box_dims=None):
        """Rule C14: the boxes of `poses` rendered into `depth` and compared with it, either a C-contiguous (F, H, W) uint16 numpy
        array (cd_verify_boxes_batch: uploaded) or a contiguous 16-bit torch tensor of that shape in HBM
        (cd_verify_boxes_batch_device; the caller has synchronised the stream that wrote it).  poses (F, B, 4, 4) float64, n_boxes
        (F,) (None: all B), cam a CdDepthCamera of that width and height, box_dims None or (F, B, 3).  Returns an array of F * B
        CdVerifyBox, box b of frame f at [f * B + b].  The images are only read."""
        ptr, on_device, F, H, W = self._depth_images(depth)
        assert (cam.width, cam.height) == (W, H)
        p = np.ascontiguousarray(poses, np.float64).reshape(F, -1, 16)
        B = p.shape[1]
        nb = np.full(F, B, np.int32) if n_boxes is None else np.ascontiguousarray(n_boxes, np.int32)
        assert nb.shape == (F,)
        dp = C.POINTER(C.c_double)
        bd = None if box_dims is None else np.ascontiguousarray(box_dims, np.float64).reshape(F, B, 3)
        out = (CdVerifyBox * max(F * B, 1))()
        fn = self.lib.cd_verify_boxes_batch_device if on_device else self.lib.cd_verify_boxes_batch
        self._check(fn(self.h, C.byref(cam), ptr, F, p.ctypes.data_as(dp), nb.ctypes.data_as(C.POINTER(C.c_int32)), B,
                       None if bd is None else bd.ctypes.data_as(dp), None if params is None else C.byref(params), out))
        return out

    def verify_last_results(self, depth, cam, which=CD_VERIFY_ACCEPTED, params=None):
        """The poses of the last fused call verified against its frames' depth images (numpy array or torch tensor as for
        verify_boxes; F = that call's frames).  which: CD_VERIFY_ACCEPTED / CD_VERIFY_ALL.  Returns F * CD_MAX_CLUSTERS_PER_FRAME
        CdVerifyBox, slot k of frame f = clusters[k] of its record.  Leaves the fused call's read-backs as they are."""
        ptr, on_device, F, H, W = self._depth_images(depth)
        assert (cam.width, cam.height) == (W, H)
        out = (CdVerifyBox * (max(F, 1) * CD_MAX_CLUSTERS_PER_FRAME))()
        fn = self.lib.cd_verify_last_results_device if on_device else self.lib.cd_verify_last_results
        self._check(fn(self.h, C.byref(cam), ptr, int(which), None if params is None else C.byref(params), out))
        return out

    def label_points_last(self, frames, out=None):
        """Rule C15: one uint8 label per input record of the LAST fused call, whose frames are passed again: a C-contiguous
        (F, P, k) float32 numpy array (cd_label_points_last; returns an (F, P) uint8 array) or a contiguous float32 torch tensor
        of that shape in HBM (cd_label_points_last_device; `out`, an (F, P) uint8 tensor on the same device, is filled and
        returned).  Leaves the fused call's read-backs as they are."""
        if isinstance(frames, np.ndarray):
            assert frames.dtype == np.float32 and frames.ndim == 3 and frames.shape[2] >= 3 and frames.flags.c_contiguous
            F, P = frames.shape[:2]
            res = np.empty((F, P), np.uint8)
            self._check(self.lib.cd_label_points_last(self.h, _ptr(frames), frames.strides[1], P, F, _ptr(res)))
            return res
        assert frames.is_contiguous() and frames.dim() == 3 and frames.element_size() == 4
        F, P = (int(v) for v in frames.shape[:2])
        assert out is not None and out.is_contiguous() and out.numel() == F * P and out.element_size() == 1
        self._check(self.lib.cd_label_points_last_device(self.h, C.c_void_p(frames.data_ptr()), 4 * int(frames.shape[2]), P, F, C.c_void_p(out.data_ptr())))
        return out

    def label_depth_last(self, depth, cam, out=None):
        """Rule C15 from the depth images of the last fused call (deprojected by rule C7): an (F, H, W) uint16 numpy array
        (cd_label_depth_last; returns the (F, H, W) uint8 label images) or a 16-bit torch tensor of that shape in HBM
        (cd_label_depth_last_device; `out`, an (F, H, W) uint8 tensor on the same device, is filled and returned)."""
        ptr, on_device, F, H, W = self._depth_images(depth)
        assert (cam.width, cam.height) == (W, H)
        if not on_device:
            res = np.empty((F, H, W), np.uint8)
            self._check(self.lib.cd_label_depth_last(self.h, C.byref(cam), ptr, F, _ptr(res)))
            return res
        assert out is not None and out.is_contiguous() and out.numel() == F * H * W and out.element_size() == 1
        self._check(self.lib.cd_label_depth_last_device(self.h, C.byref(cam), ptr, F, C.c_void_p(out.data_ptr())))
        return out

    def tint_labels(self, rgb, labels, palette=None):
        """cd_tint_labels_batch[_device]: the labels drawn IN PLACE over rgb, an (F, H, W, 3) uint8 numpy array with (F, H, W)
        uint8 numpy labels, or torch tensors of those shapes in HBM.  palette: None (the default) or a (256, 4) uint8 array."""
        pal = None
        if palette is not None:
            pal = CdLabelPalette.from_buffer_copy(np.ascontiguousarray(palette, np.uint8).reshape(256, 4).tobytes())
        on_device = not isinstance(rgb, np.ndarray)
        F, H, W = (int(v) for v in rgb.shape[:3])
        if on_device:
            assert rgb.is_contiguous() and rgb.dim() == 4 and rgb.shape[3] == 3 and labels.is_contiguous() and labels.numel() == F * H * W
            a, b = C.c_void_p(rgb.data_ptr()), C.c_void_p(labels.data_ptr())
        else:
            assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3 and rgb.flags.c_contiguous and rgb.flags.writeable
            assert labels.dtype == np.uint8 and labels.size == F * H * W and labels.flags.c_contiguous
            a, b = _ptr(rgb), _ptr(labels)
        fn = self.lib.cd_tint_labels_batch_device if on_device else self.lib.cd_tint_labels_batch
        self._check(fn(self.h, a, b, W, H, F, None if pal is None else C.byref(pal)))
        return rgb

    def surface_batch(self, clouds, table_normals, prm, invert=True):
        """cd_surface_batch: cd_surface_frame over a batch of (ragged) clouds, fitted together on the device.
        clouds: a sequence of (n_f, >=3) arrays or an (F, P, >=3) array; table_normals (F, 3).
        Returns (frame_status int32[F], CdSurfaceFrameResult array of F)."""
        clouds = [np.asarray(c, np.float32).reshape(-1, np.shape(c)[-1]) for c in clouds]
        F = len(clouds)
        counts = np.array([c.shape[0] for c in clouds], np.int32)
        P = max(1, int(counts.max()) if F else 1)
        packed = np.zeros((F, P, 4), np.float32)
        for f, c in enumerate(clouds):
            packed[f, :c.shape[0], :3] = c[:, :3]
        tn = np.ascontiguousarray(table_normals, np.float32).reshape(F, 3)
        out = (CdSurfaceFrameResult * max(F, 1))()
        status = np.zeros(max(F, 1), np.int32)
        i32 = C.POINTER(C.c_int32)
        st = self.lib.cd_surface_batch(self.h, _ptr(packed), 16, P, counts.ctypes.data_as(i32), F,
                                       tn.ctypes.data_as(C.POINTER(C.c_float)), 1 if invert else 0, C.byref(prm), out,
                                       status.ctypes.data_as(i32))
        self._check(st)
        return status[:F], out

    def surface_results(self):
        """cd_get_surface_results: the per-frame surface results of the last CD_GUESS_SURFACE fused call.
        Returns (frame_status int32[F], CdSurfaceFrameResult array of F)."""
        out = (CdSurfaceFrameResult * self.max_frames)()
        status = np.zeros(self.max_frames, np.int32)
        n = self.lib.cd_get_surface_results(self.h, 0, self.max_frames, out, status.ctypes.data_as(C.POINTER(C.c_int32)))
        if n < 0:
            raise CuboidError(n, "cd_get_surface_results: the last fused call was not in CD_GUESS_SURFACE mode")
        return status[:n].copy(), out[:n]

    def set_surface_distance_threshold(self, d):
        """sne's distance threshold for CD_GUESS_SURFACE (context state; default 0.015)."""
        self._check(self.lib.cd_set_surface_distance_threshold(self.h, float(d)))

    def surface_distance_threshold(self):
        v = C.c_double()
        self._check(self.lib.cd_get_surface_distance_threshold(self.h, C.byref(v)))
        return v.value

    def set_icp_max_correspondence_distance(self, d):
        """IterativeClosestPoint::setMaxCorrespondenceDistance for every later ICP of this context (rule C8); None = unbounded."""
        self._check(self.lib.cd_set_icp_max_correspondence_distance(self.h, float("inf") if d is None else float(d)))

    def icp_max_correspondence_distance(self):
        """The distance as set (+inf: unbounded, the default)."""
        v = C.c_double()
        self._check(self.lib.cd_get_icp_max_correspondence_distance(self.h, C.byref(v)))
        return v.value

    def set_outlier_filter(self, mean_k, std_mul=1.0, negative=False):
        """Rule C16 (pcl::StatisticalOutlierRemoval) on the object cloud of the following fused calls; mean_k = 0 (or None): off."""
        self._check(self.lib.cd_set_outlier_filter(self.h, int(mean_k or 0), float(std_mul), 1 if negative else 0))

    def outlier_filter_setting(self):
        """(mean_k, std_mul, negative) as cd_set_outlier_filter left them; mean_k = 0: off."""
        k, neg, mul = C.c_int(), C.c_int(), C.c_double()
        self._check(self.lib.cd_get_outlier_filter(self.h, C.byref(k), C.byref(mul), C.byref(neg)))
        return k.value, mul.value, bool(neg.value)

    def outlier_stats(self, frame):
        """What the filter did to `frame` of the last fused call: dict(n_before, n_removed, mean, stddev, threshold)."""
        nb, nr = C.c_int(), C.c_int()
        mean, sd, thr = C.c_double(), C.c_double(), C.c_double()
        st = self.lib.cd_get_outlier_stats(self.h, frame, C.byref(nb), C.byref(nr), C.byref(mean), C.byref(sd), C.byref(thr))
        if st != CD_OK:
            raise CuboidError(st, "no filtered fused call to read: the last one ran without the filter, has been invalidated, or had no such frame")
        return dict(n_before=nb.value, n_removed=nr.value, mean=mean.value, stddev=sd.value, threshold=thr.value)

    def outlier_filter(self, xyz, mean_k, std_mul=1.0, negative=False, capacity=None):
        """The filter as a call of its own.  Returns (kept indices int32 ascending, dist float32 (n), (mean, stddev, threshold))."""
        a, stride, n = _points(xyz)
        cap = max(n, 1) if capacity is None else int(capacity)
        idx = np.empty(max(cap, 1), np.int32)
        dist = np.zeros(max(n, 1), np.float32)
        stats = np.zeros(3, np.float64)
        cnt = C.c_int()
        self._check(self.lib.cd_outlier_filter(self.h, _ptr(a), stride, n, int(mean_k), float(std_mul), 1 if negative else 0, _ptr(idx), cap,
                                               C.byref(cnt), _ptr(dist), _ptr(stats)))
        return idx[:cnt.value].copy(), dist[:n].copy(), tuple(float(v) for v in stats)

    def set_table_prism(self, enable, height_min=0.0, height_max=0.5):
        """Rule C20 (pcl::ConvexHull of the plane inliers + pcl::ExtractPolygonalPrismData) on the object cloud of the following
        fused calls, ahead of the outlier filter; enable false: off, the default."""
        self._check(self.lib.cd_set_table_prism(self.h, 1 if enable else 0, float(height_min), float(height_max)))

    def table_prism_setting(self):
        """(enable, height_min, height_max) as cd_set_table_prism left them."""
        on, lo, hi = C.c_int(), C.c_double(), C.c_double()
        self._check(self.lib.cd_get_table_prism(self.h, C.byref(on), C.byref(lo), C.byref(hi)))
        return bool(on.value), lo.value, hi.value

    def prism_stats(self, frame):
        """What the table prism did to `frame` of the last fused call: a dict of cd_prism_stats' fields."""
        out = CdPrismStats()
        st = self.lib.cd_get_prism_stats(self.h, frame, C.byref(out))
        if st != CD_OK:
            raise CuboidError(st, "no fused call with the table prism to read: the last one ran without it, has been invalidated, or had no such frame")
        return out.as_dict()

    def prism_hull(self, frame):
        """The hull of `frame` of the last fused call: (hull_vertices, 2) int32, counter-clockwise from the lexicographically smallest."""
        uv = np.zeros((CD_PRISM_MAX_HULL, 2), np.int32)
        n = C.c_int()
        self._check(self.lib.cd_get_prism_hull(self.h, frame, _ptr(uv), CD_PRISM_MAX_HULL, C.byref(n)))
        return uv[:n.value].copy()

    def table_prism(self, plane_xyz, coeff, xyz, height_min=0.0, height_max=0.5, capacity=None):
        """The step as a call of its own.  Returns (kept indices int32 ascending, a dict of cd_prism_stats' fields, hull (h, 2) int32)."""
        pl, pstride, npl = _points(np.asarray(plane_xyz, np.float32).reshape(-1, 3) if np.size(plane_xyz) == 0 else plane_xyz)
        a, stride, n = _points(np.asarray(xyz, np.float32).reshape(-1, 3) if np.size(xyz) == 0 else xyz)
        cf = np.ascontiguousarray(coeff, np.float32).reshape(4)
        cap = max(n, 1) if capacity is None else int(capacity)
        idx = np.empty(max(cap, 1), np.int32)
        uv = np.zeros((CD_PRISM_MAX_HULL, 2), np.int32)
        stats = CdPrismStats()
        cnt = C.c_int()
        self._check(self.lib.cd_table_prism(self.h, _ptr(pl), pstride, npl, _ptr(cf), _ptr(a), stride, n, float(height_min), float(height_max),
                                            _ptr(idx), cap, C.byref(cnt), C.byref(stats), _ptr(uv), CD_PRISM_MAX_HULL))
        return idx[:cnt.value].copy(), stats.as_dict(), uv[:stats.hull_vertices].copy()

    def set_icp_plane_weight(self, tangent_weight, switch_distance=CD_ICP_PLANE_SWITCH_DEFAULT):
        """Rule C17, the plane-weighted ICP step for lattice templates, for every later ICP of this context; tangent_weight = 0
        (or None): off, the default.  The recommended pair is (CD_ICP_PLANE_WEIGHT_DEFAULT, CD_ICP_PLANE_SWITCH_DEFAULT)."""
        self._check(self.lib.cd_set_icp_plane_weight(self.h, float(tangent_weight or 0.0), float(switch_distance)))

    def icp_plane_weight(self):
        """(tangent_weight, switch_distance) as cd_set_icp_plane_weight left them; tangent_weight = 0: off."""
        w, d = C.c_double(), C.c_double()
        self._check(self.lib.cd_get_icp_plane_weight(self.h, C.byref(w), C.byref(d)))
        return w.value, d.value

    def _cluster_records(self, fn, ctype, message, frame, first, count, default_count=4096):
        """The read-backs of one record per cluster (cd_get_cluster_*_stats, cd_get_cluster_shape_frames): up to `count` records
        of `frame` from its cluster `first` on, as a list of `ctype`; a negative return raises CuboidError with `message`."""
        cap = default_count if count is None else int(count)
        out = (ctype * max(cap, 1))()
        got = fn(self.h, frame, first, cap, out)
        if got < 0:
            raise CuboidError(got, message)
        return out[:got]

    def cluster_plane_stats(self, frame, first=0, count=None):
        """Rule C17's counters of the clusters of `frame` of the last fused call (or, frame 0, of the last cd_icp), indexed like
        cluster_results: an (n, 4) int32 array of plane_iterations, first_plane_iteration, stopped_singular, reserved."""
        msg = "no plane-weighted call to read: the last one ran with the mode off, has been invalidated, or had no such frame"
        rows = self._cluster_records(self.lib.cd_get_cluster_plane_stats, C.c_int32 * 4, msg, frame, first, count)
        return np.array([r[:] for r in rows], np.int32).reshape(-1, 4)

    def set_icp_coarse(self, stride, min_points=0):
        """Rule C18, coarse-to-fine ICP, for every later ICP of this context: pairs whose cluster has at least min_points points
        first register every stride-th point, then all points from that pose.  stride = 0 (or None): off, the default."""
        self._check(self.lib.cd_set_icp_coarse(self.h, int(stride or 0), int(min_points)))

    def icp_coarse(self):
        """(stride, min_points) as cd_set_icp_coarse left them; stride = 0: off."""
        s, m = C.c_int(), C.c_int()
        self._check(self.lib.cd_get_icp_coarse(self.h, C.byref(s), C.byref(m)))
        return s.value, m.value

    def cluster_coarse_stats(self, frame, first=0, count=None):
        """Rule C18's stats of the clusters of `frame` of the last fused call (or, frame 0, of the last cd_icp), indexed like
        cluster_results: a list of CdIcpCoarseStats."""
        msg = "no coarse-to-fine call to read: the last one ran with the mode off, has been invalidated, or had no such frame"
        return self._cluster_records(self.lib.cd_get_cluster_coarse_stats, CdIcpCoarseStats, msg, frame, first, count)

    def set_icp_median_rejection(self, factor):
        """Rule C19, median-distance correspondence rejection, for every later ICP of this context: an iteration keeps the
        correspondences whose squared distance is at most factor times the upper median.  factor = 0 (or None): off, the default."""
        self._check(self.lib.cd_set_icp_median_rejection(self.h, 0.0 if factor is None else float(factor)))

    def icp_median_rejection(self):
        """The factor as cd_set_icp_median_rejection left it; 0: off."""
        f = C.c_double()
        self._check(self.lib.cd_get_icp_median_rejection(self.h, C.byref(f)))
        return f.value

    def cluster_reject_stats(self, frame, first=0, count=None):
        """Rule C19's stats of the clusters of `frame` of the last fused call (or, frame 0, of the last cd_icp), indexed like
        cluster_results: a list of CdIcpRejectStats."""
        msg = "no median-rejection call to read: the last one ran with the mode off, has been invalidated, or had no such frame"
        return self._cluster_records(self.lib.cd_get_cluster_reject_stats, CdIcpRejectStats, msg, frame, first, count)

    def set_icp_reciprocal(self, on):
        """Rule C22, reciprocal correspondences, for every later ICP of this context: an iteration keeps a source point's template
        neighbour only if that template point's nearest source point is the same source point.  False (or None): off, the default."""
        self._check(self.lib.cd_set_icp_reciprocal(self.h, 1 if on else 0))

    def icp_reciprocal(self):
        """The mode as cd_set_icp_reciprocal left it: 1 on, 0 off."""
        v = C.c_int()
        self._check(self.lib.cd_get_icp_reciprocal(self.h, C.byref(v)))
        return v.value

    def cluster_recip_stats(self, frame, first=0, count=None):
        """Rule C22's stats of the clusters of `frame` of the last fused call (or, frame 0, of the last cd_icp), indexed like
        cluster_results: a list of CdIcpRecipStats."""
        msg = "no reciprocal-correspondence call to read: the last one ran with the mode off, has been invalidated, or had no such frame"
        return self._cluster_records(self.lib.cd_get_cluster_recip_stats, CdIcpRecipStats, msg, frame, first, count)

    def set_pair_score(self, enable, max_range=CD_PAIR_SCORE_RANGE_DEFAULT, min_coverage=CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT,
                       min_inlier_fraction=CD_PAIR_SCORE_MIN_INLIER_DEFAULT):
        """Rule C21, the two-way registration score, for every later fused call of this context: each cluster result is scored
        against the template it reports (coverage of the template, inlier fraction, bounded fitnesses, `valid`).  Off by default."""
        self._check(self.lib.cd_set_pair_score(self.h, 1 if enable else 0, float(max_range), float(min_coverage), float(min_inlier_fraction)))

    def pair_score_setting(self):
        """(enable, max_range, min_coverage, min_inlier_fraction) as cd_set_pair_score left them."""
        on, d, a, b = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.cd_get_pair_score(self.h, C.byref(on), C.byref(d), C.byref(a), C.byref(b)))
        return on.value, d.value, a.value, b.value

    def cluster_pair_scores(self, frame, first=0, count=None):
        """Rule C21's records of the clusters of `frame` of the last fused call, indexed like cluster_results: a list of CdPairScore."""
        msg = "no pair-score call to read: the last fused call ran with the mode off, has been invalidated, or had no such frame"
        return self._cluster_records(self.lib.cd_get_cluster_pair_scores, CdPairScore, msg, frame, first, count)

    def pair_score_points(self, slot, src, T, max_range=CD_PAIR_SCORE_RANGE_DEFAULT, min_coverage=CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT,
                          min_inlier_fraction=CD_PAIR_SCORE_MIN_INLIER_DEFAULT, accepted=1):
        """One pair on the GPU without a fused call: src (n, >= 3) float32 against the template of `slot` under T.  Returns a dict
        of cd_pair_score's fields (its own status in "status")."""
        src = np.asarray(src, np.float32)
        a, stride, n = _points(src if src.ndim == 2 else src.reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = CdPairScore()
        self._check(self.lib.cd_pair_score_points(self.h, int(slot), _ptr(a), stride, n, _ptr(t), float(max_range), float(min_coverage),
                                                  float(min_inlier_fraction), 1 if accepted else 0, C.byref(out)))
        return out.as_dict()

    def set_pose_info(self, enable, max_range=CD_POSE_INFO_RANGE_DEFAULT, min_support=CD_POSE_INFO_MIN_SUPPORT_DEFAULT):
        """Rule C23, the pose information, for every later fused call of this context: each cluster result gets the eigenvalues of its
        information matrix over a small rigid motion ("points' worth" per direction), n_constrained, well_posed and the covariance of
        the pose.  Lattice templates only.  Off by default."""
        self._check(self.lib.cd_set_pose_info(self.h, 1 if enable else 0, float(max_range), float(min_support)))

    def pose_info_setting(self):
        """(enable, max_range, min_support) as cd_set_pose_info left them."""
        on, d, s = C.c_int(), C.c_double(), C.c_double()
        self._check(self.lib.cd_get_pose_info(self.h, C.byref(on), C.byref(d), C.byref(s)))
        return on.value, d.value, s.value

    def cluster_pose_info(self, frame, first=0, count=None):
        """Rule C23's records of the clusters of `frame` of the last fused call, indexed like cluster_results: a list of CdPoseInfo."""
        msg = "no pose-information call to read: the last fused call ran with the mode off, has been invalidated, or had no such frame"
        return self._cluster_records(self.lib.cd_get_cluster_pose_info, CdPoseInfo, msg, frame, first, count)

    def pose_info_points(self, slot, src, T, max_range=CD_POSE_INFO_RANGE_DEFAULT, min_support=CD_POSE_INFO_MIN_SUPPORT_DEFAULT, accepted=1):
        """One pair on the GPU without a fused call: src (n, >= 3) float32 against the lattice template of `slot` under T.  Returns a
        dict of cd_pose_info's fields (its own status in "status")."""
        src = np.asarray(src, np.float32)
        a, stride, n = _points(src if src.ndim == 2 else src.reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = CdPoseInfo()
        self._check(self.lib.cd_pose_info_points(self.h, int(slot), _ptr(a), stride, n, _ptr(t), float(max_range), float(min_support),
                                                 1 if accepted else 0, C.byref(out)))
        return out.as_dict()

    def set_box_fit(self, enable, band=CD_BOX_FIT_BAND_DEFAULT):
        """Rule C24, the box fit, for every later fused call of this context: each cluster gets the dimensions, pose and rectangularity
        of the cuboid it is the view of, from its points and the frame's plane alone.  Off by default."""
        self._check(self.lib.cd_set_box_fit(self.h, 1 if enable else 0, float(band)))

    def box_fit_setting(self):
        """(enable, band) as cd_set_box_fit left them."""
        on, b = C.c_int(), C.c_double()
        self._check(self.lib.cd_get_box_fit(self.h, C.byref(on), C.byref(b)))
        return on.value, b.value

    def set_box_select(self, enable, slot_dims=None, tolerance=0.0):
        """The selection of rule C24 for every later fused call with template_slot = -1: a cluster whose box record matches the
        dimensions of a loaded slot (slot_dims: up to CD_MAX_TEMPLATES rows of length, width, height) within the tolerance is
        registered against that slot alone.  Needs set_box_fit(True).  Off by default."""
        sd = np.zeros((CD_MAX_TEMPLATES, 3), np.float64)
        if slot_dims is not None:
            rows = np.asarray(slot_dims, np.float64).reshape(-1, 3)
            sd[:len(rows)] = rows
        self._check(self.lib.cd_set_box_select(self.h, 1 if enable else 0, _ptr(sd), float(tolerance)))

    def box_select_setting(self):
        """(enable, slot_dims (CD_MAX_TEMPLATES, 3), tolerance) as cd_set_box_select left them."""
        on, tol, sd = C.c_int(), C.c_double(), np.zeros((CD_MAX_TEMPLATES, 3), np.float64)
        self._check(self.lib.cd_get_box_select(self.h, C.byref(on), _ptr(sd), C.byref(tol)))
        return on.value, sd, tol.value

    def cluster_box_fits(self, frame, first=0, count=None):
        """Rule C24's records of the clusters of `frame` of the last fused call, indexed like cluster_results: a list of CdBoxFit."""
        msg = "no box-fit call to read: the last fused call ran with the step off, has been invalidated, or had no such frame"
        return self._cluster_records(self.lib.cd_get_cluster_box_fits, CdBoxFit, msg, frame, first, count)

    def box_fit_points(self, coeffs, sets, band=CD_BOX_FIT_BAND_DEFAULT):
        """Rule C24 on the device without a fused call: one dict of cd_box_fit's fields per point set of `sets` (a sequence of
        (n_i, 3) float32 arrays) against the plane coeffs[i] (4 float32), all in one launch (cd_box_fit_points)."""
        sets = [np.asarray(a, np.float32).reshape(-1, 3) for a in sets]
        co = np.ascontiguousarray(np.asarray(coeffs, np.float32).reshape(len(sets), 4))
        pts = np.ascontiguousarray(np.concatenate(sets, axis=0))
        off = np.zeros(len(sets) + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in sets])
        out = (CdBoxFit * len(sets))()
        self._check(self.lib.cd_box_fit_points(self.h, _ptr(co), _ptr(pts), 12, off.ctypes.data_as(C.POINTER(C.c_int32)), len(sets), float(band), out))
        return [r.as_dict() for r in out]

    def passthrough(self, records, field, lo, hi, negative=False):
        """pcl::PassThrough on whole records: `records` (n, k >= 3) of 4-byte items; field 'x' / 'y' / 'z' or None."""
        r = np.ascontiguousarray(records)
        assert r.ndim == 2 and r.dtype.itemsize == 4 and r.shape[1] >= 3
        out = np.empty_like(r)
        cnt = C.c_int()
        f = -1 if field is None else "xyz".index(field)
        self._check(self.lib.cd_passthrough(self.h, _ptr(r), r.shape[1] * 4, r.shape[0], f, float(lo), float(hi), 1 if negative else 0,
                                            _ptr(out), r.shape[0], C.byref(cnt)))
        return out[:cnt.value].copy()

    def template_lattice_faces(self, slot):
        """Faces of the slot's template as a union of axis-aligned lattices (make_cuboid.py's output); 0 = an arbitrary cloud."""
        return self._check(self.lib.cd_template_lattice_faces(self.h, slot), ok=tuple(range(0, 9)))

    def template_nearest(self, slot, queries):
        """Nearest template point of every query: (original index int32, squared distance float32).  Lattice templates only."""
        a, stride, n = _points(queries)
        idx = np.empty(max(n, 1), np.int32)
        d2 = np.empty(max(n, 1), np.float32)
        self._check(self.lib.cd_template_nearest(self.h, slot, _ptr(a), stride, n, _ptr(idx), _ptr(d2)))
        return idx[:n], d2[:n]

    def depth_to_cloud(self, cam, depth, color=None, stride_bytes=16, rgb_offset=12, color_camera=None):
        """One depth image (H, W) uint16 (+ colour (H, W, 3) uint8 when cam.color is CD_COLOR_RGB8) -> the organized cloud as
        (W * H, stride_bytes / 4) uint32 records: x,y,z at words 0..2 (NaN where the depth is 0), the packed rgb at rgb_offset
        (-1: none), the rest zero.  color_camera (a CdColorCamera): the pair is UNREGISTERED - colour is (ch, cw, 3) at the colour
        camera's size and the cloud is built by rule C12 (cd_depth_to_cloud_mapped)."""
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        c = None if color is None else np.ascontiguousarray(color, dtype=np.uint8)
        n = int(cam.width) * int(cam.height)
        out = np.zeros((max(n, 1), stride_bytes // 4), np.uint32)
        cnt = C.c_int()
        if color_camera is not None:
            self._check(self.lib.cd_depth_to_cloud_mapped(self.h, C.byref(cam), C.byref(color_camera), _ptr(d), _ptr(c), _ptr(out),
                                                          stride_bytes, rgb_offset, n, C.byref(cnt)))
            return out[:cnt.value]
        self._check(self.lib.cd_depth_to_cloud(self.h, C.byref(cam), _ptr(d), _ptr(c), _ptr(out), stride_bytes, rgb_offset, n,
                                               C.byref(cnt)))
        return out[:cnt.value]

    def _depth_call(self, color_camera, device, cam, depth_ptr, color_ptr, n_frames, prm, res, pi, lb):
        """cd_process_depth_batch[_device], or with a colour camera cd_process_depth_batch_mapped[_device]."""
        tail = (depth_ptr, color_ptr, n_frames, C.byref(prm), C.cast(res, C.c_void_p), _ptr(pi), _ptr(lb))
        if color_camera is None:
            fn = self.lib.cd_process_depth_batch_device if device else self.lib.cd_process_depth_batch
            return self._check(fn(self.h, C.byref(cam), *tail))
        fn = self.lib.cd_process_depth_batch_mapped_device if device else self.lib.cd_process_depth_batch_mapped
        return self._check(fn(self.h, C.byref(cam), C.byref(color_camera), *tail))

    def process_depth_batch(self, depth, color, cam, prm, want_indices=False, color_camera=None):
        """depth (F, H, W) uint16, color (F, H, W, 3) uint8 or None (cam.color decides whether it is read): the chain on the
        organized clouds the images deproject to.  Returns (results, plane_inliers, labels) as process_batch does.
        color_camera: the pairs are unregistered, color is (F, ch, cw, 3) (rule C12, cd_process_depth_batch_mapped)."""
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        assert d.ndim == 3
        c = None if color is None else np.ascontiguousarray(color, dtype=np.uint8)
        F, N = d.shape[0], d.shape[1] * d.shape[2]
        res = (CdFrameResult * F)()
        pi = np.empty((F, N), np.int32) if want_indices else None
        lb = np.empty((F, N), np.int32) if want_indices else None
        self._depth_call(color_camera, False, cam, _ptr(d), _ptr(c), F, prm, res, pi, lb)
        return res, pi, lb

    def process_depth_batch_device(self, depth, color, cam, prm, results=None, plane_inliers=None, labels=None, color_camera=None):
        """depth: contiguous torch uint16 tensor (F, H, W) in HBM, color: uint8 tensor (F, H, W, 3) or None (data_ptr(); the
        caller has synchronised the stream that wrote them, as for process_batch_device).  color_camera: as process_depth_batch."""
        assert depth.is_contiguous() and depth.dim() == 3 and (color is None or color.is_contiguous())
        F = depth.shape[0]
        res = results if results is not None else (CdFrameResult * F)()
        self._depth_call(color_camera, True, cam, C.c_void_p(depth.data_ptr()), None if color is None else C.c_void_p(color.data_ptr()),
                         F, prm, res, plane_inliers, labels)
        return res

    def process_depth_batch_host_ptr(self, depth_ptr, color_ptr, n_frames, cam, prm, results=None, color_camera=None):
        """cd_process_depth_batch on raw HOST pointers (e.g. pinned torch tensors' data_ptr()): the uploads are part of the call.
        color_camera: as process_depth_batch."""
        res = results if results is not None else (CdFrameResult * n_frames)()
        self._depth_call(color_camera, False, cam, C.c_void_p(depth_ptr), C.c_void_p(color_ptr) if color_ptr else None, n_frames, prm,
                         res, None, None)
        return res

    def shape_frames(self, sets):
        """Rule C13 on the device: one CdShapeFrame per point set of `sets` (a sequence of (n_i, >= 3) float32 arrays that share
        their number of columns, i.e. their stride), all in one launch (cd_shape_frames)."""
        sets = [np.asarray(a, np.float32) for a in sets]
        cols = sets[0].shape[1]
        assert all(a.ndim == 2 and a.shape[1] == cols for a in sets)
        pts = np.ascontiguousarray(np.concatenate(sets, axis=0))
        off = np.zeros(len(sets) + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in sets])
        out = (CdShapeFrame * len(sets))()
        self._check(self.lib.cd_shape_frames(self.h, _ptr(pts), cols * 4, off.ctypes.data_as(C.POINTER(C.c_int32)), len(sets), out))
        return out

    def template_shape_frame(self, slot):
        """The record cd_set_template computed for the slot's template (rule C13)."""
        r = CdShapeFrame()
        self._check(self.lib.cd_template_shape_frame(self.h, slot, C.byref(r)))
        return r

    def cluster_shape_frames(self, frame, first=0, count=None):
        """The cluster records of `frame` of the last fused call in CD_GUESS_CLUSTER mode: a list of CdShapeFrame."""
        msg = "cd_get_cluster_shape_frames: the last fused call was not in CD_GUESS_CLUSTER mode"
        return self._cluster_records(self.lib.cd_get_cluster_shape_frames, CdShapeFrame, msg, frame, first, count, CD_MAX_CLUSTERS_PER_FRAME * 64)

    def timing(self):
        t = CdTiming()
        self._check(self.lib.cd_get_timing(self.h, C.byref(t)))
        return t


def lattice_detect(xyz):
    """Host-only lattice test of cd_set_template: list of faces (constant axis, fast axis, first index, n_fast, n_slow)."""
    lib = load_library()
    a, stride, m = _points(xyz)
    out = np.zeros((8, 5), np.int32)
    nf = lib.cd_lattice_detect(_ptr(a), stride, m, _ptr(out))
    if nf < 0:
        raise CuboidError(nf, "cd_lattice_detect")
    return [tuple(int(v) for v in out[f]) for f in range(nf)]


def lattice_axes(xyz):
    """Host-only: (axes_distinct, axis_face[3], axis_c[3]) of the lattice cd_lattice_detect finds - at most one face per constant
    axis (1) or not (0, also for points that are no lattice); face index per axis (-1: none) and its constant coordinate (NaN)."""
    lib = load_library()
    a, stride, m = _points(xyz)
    face = np.zeros(3, np.int32)
    c = np.zeros(3, np.float32)
    r = lib.cd_lattice_axes(_ptr(a), stride, m, _ptr(face), _ptr(c))
    if r < 0:
        raise CuboidError(r, "cd_lattice_axes")
    return int(r), [int(v) for v in face], c


ICP_STATE = np.dtype([("Tfinal", np.float32, 16), ("T", np.float32, 16), ("prev_mse", np.float64), ("iters", np.int32),
                      ("done", np.int32), ("converged", np.int32), ("status", np.int32)])


def icp_solve_batch(sums, n, states, max_iter=50, trans_eps=1e-8, rel_mse=1e-6, rot_thr=None, abs_mse=1e-12, bounded=False, unary=False):
    """cd_icp_solve_batch: one ICP step for k records (sums uint64 [k, 16], n int32 [k], states ICP_STATE [k]) by the row code
    and by the single-lane code in one launch.  Returns (states_row, states_lane, done int32 [k, 2], unary uint64 [6] or None)."""
    lib = load_library()
    sums = np.ascontiguousarray(sums, np.uint64).reshape(-1, 16)
    k = sums.shape[0]
    n = np.ascontiguousarray(n, np.int32).reshape(k)
    states = np.ascontiguousarray(states, ICP_STATE).reshape(k)
    out_row, out_lane = np.zeros(k, ICP_STATE), np.zeros(k, ICP_STATE)
    done = np.zeros((k, 2), np.int32)
    un = np.zeros(6, np.uint64) if unary else None
    st = lib.cd_icp_solve_batch(k, _ptr(sums), _ptr(n), _ptr(states), int(max_iter), float(trans_eps), float(rel_mse),
                                float(1.0 - trans_eps if rot_thr is None else rot_thr), float(abs_mse), int(bool(bounded)),
                                _ptr(out_row), _ptr(out_lane), _ptr(done), None if un is None else _ptr(un))
    if st != CD_OK:
        raise CuboidError(st, "cd_icp_solve_batch")
    return out_row, out_lane, done, un


def icp_coarse_subsample(n, stride, min_points, capacity=None):
    """Host only: rule C18's coarse indices of a set of n points (int32; empty when the set is not eligible).  capacity: the
    buffer handed to the library (default: as many as it needs); a count over it returns (count, None)."""
    lib = load_library()
    need = lib.cd_icp_coarse_subsample(int(n), int(stride), int(min_points), None, 0)
    if capacity is None:
        capacity = need
    out = np.zeros(max(int(capacity), 1), np.int32)
    got = lib.cd_icp_coarse_subsample(int(n), int(stride), int(min_points), _ptr(out), int(capacity))
    if got > capacity:
        return got, None
    return out[:got].copy()


def icp_median_threshold(d2, factor):
    """Host-only rule C19, steps 2 and 3: (m float32, thr float64) of the squared distances of K0."""
    lib = load_library()
    a = np.ascontiguousarray(d2, np.float32).reshape(-1)
    m, t = C.c_float(), C.c_double()
    st = lib.cd_icp_median_threshold(_ptr(a), len(a), float(factor), C.byref(m), C.byref(t))
    if st != CD_OK:
        raise CuboidError(st, "cd_icp_median_threshold")
    return np.float32(m.value), np.float64(t.value)


def icp_reciprocal_mask(src, tpl, d2_max=None):
    """Host-only rule C22, steps 1 - 3 of one iteration by brute force: (nn int32, d2 float32, keep bool, n0) for the source
    positions src over the template tpl; d2_max: rule C8's float32 threshold on d2 (None: unbounded)."""
    lib = load_library()
    s = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(tpl, np.float32).reshape(-1, 3))
    nn = np.empty(len(s), np.int32)
    d2 = np.empty(len(s), np.float32)
    keep = np.empty(len(s), np.uint8)
    n0 = lib.cd_icp_reciprocal_mask(_ptr(s), 12, len(s), _ptr(t), 12, len(t), float("inf") if d2_max is None else float(np.float32(d2_max)), _ptr(nn), _ptr(d2),
                                    _ptr(keep))
    if n0 < 0:
        raise CuboidError(n0, "cd_icp_reciprocal_mask")
    return nn, d2, keep.astype(bool), n0


def pair_score_host(tpl, src, T, max_range=CD_PAIR_SCORE_RANGE_DEFAULT, min_coverage=CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT,
                    min_inlier_fraction=CD_PAIR_SCORE_MIN_INLIER_DEFAULT, accepted=1):
    """cd_pair_score_host: rule C21 on the host (no context, no GPU).  Returns a dict of cd_pair_score's fields."""
    lib = load_library()
    tp = np.ascontiguousarray(np.asarray(tpl, np.float32).reshape(-1, 3))
    sp = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
    out = CdPairScore()
    st = lib.cd_pair_score_host(_ptr(tp), 12, len(tp), _ptr(sp), 12, len(sp), _ptr(t), float(max_range), float(min_coverage),
                                float(min_inlier_fraction), 1 if accepted else 0, C.byref(out))
    if st != CD_OK:
        raise CuboidError(st, "cd_pair_score_host")
    return out.as_dict()


def pose_info_host(tpl, src, T, max_range=CD_POSE_INFO_RANGE_DEFAULT, min_support=CD_POSE_INFO_MIN_SUPPORT_DEFAULT, accepted=1):
    """cd_pose_info_host: rule C23 on the host (no context, no GPU).  Returns a dict of cd_pose_info's fields."""
    lib = load_library()
    tp = np.ascontiguousarray(np.asarray(tpl, np.float32).reshape(-1, 3))
    sp = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
    out = CdPoseInfo()
    st = lib.cd_pose_info_host(_ptr(tp), 12, len(tp), _ptr(sp), 12, len(sp), _ptr(t), float(max_range), float(min_support), 1 if accepted else 0, C.byref(out))
    if st != CD_OK:
        raise CuboidError(st, "cd_pose_info_host")
    return out.as_dict()


def pose_info_ros_covariance(info, T):
    """cd_pose_info_ros_covariance: the (6, 6) float64 covariance of the published pose P = T^-1 in geometry_msgs/PoseWithCovariance
    order from a record (a CdPoseInfo or a dict of its fields)."""
    lib = load_library()
    if not isinstance(info, CdPoseInfo):
        rec = CdPoseInfo()
        for k, _ in CdPoseInfo._fields_:
            v = info[k]
            if hasattr(v, "__len__"):
                for i, x in enumerate(v):
                    getattr(rec, k)[i] = x
            else:
                setattr(rec, k, v)
        info = rec
    t = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
    out = np.zeros(36, np.float64)
    st = lib.cd_pose_info_ros_covariance(C.byref(info), _ptr(t), _ptr(out))
    if st != CD_OK:
        raise CuboidError(st, "cd_pose_info_ros_covariance")
    return out.reshape(6, 6)


def box_fit_host(coeff, xyz, band=CD_BOX_FIT_BAND_DEFAULT):
    """cd_box_fit_host: rule C24 on the host (no context, no GPU).  Returns a dict of cd_box_fit's fields."""
    lib = load_library()
    co = np.ascontiguousarray(np.asarray(coeff, np.float32).reshape(4))
    p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    out = CdBoxFit()
    st = lib.cd_box_fit_host(_ptr(co), _ptr(p), 12, len(p), float(band), C.byref(out))
    if st != CD_OK:
        raise CuboidError(st, "cd_box_fit_host")
    return out.as_dict()


def box_fit_match(dims, slot_dims, loaded_mask, tolerance):
    """cd_box_fit_match: (slot, cost) of the fitted dims (3) against slot_dims (up to CD_MAX_TEMPLATES rows of length, width, height)."""
    lib = load_library()
    d = np.ascontiguousarray(np.asarray(dims, np.float64).reshape(3))
    sd = np.zeros((CD_MAX_TEMPLATES, 3), np.float64)
    rows = np.asarray(slot_dims, np.float64).reshape(-1, 3)
    sd[:len(rows)] = rows
    slot, cost = C.c_int32(), C.c_double()
    st = lib.cd_box_fit_match(_ptr(d), _ptr(sd), int(loaded_mask) & ((1 << CD_MAX_TEMPLATES) - 1), float(tolerance), C.byref(slot), C.byref(cost))
    if st != CD_OK:
        raise CuboidError(st, "cd_box_fit_match")
    return slot.value, cost.value


def prism_project(coeff, xyz):
    """Host-only rule C20, steps 1 - 5 of one point: (height float64, (u, v), (k1, k2))."""
    lib = load_library()
    cf = np.ascontiguousarray(coeff, np.float32).reshape(4)
    p = np.ascontiguousarray(xyz, np.float32).reshape(3)
    h = C.c_double()
    uv, ax = np.zeros(2, np.int32), np.zeros(2, np.int32)
    st = lib.cd_prism_project(_ptr(cf), _ptr(p), C.byref(h), _ptr(uv), _ptr(ax))
    if st != CD_OK:
        raise CuboidError(st, "cd_prism_project")
    return np.float64(h.value), (int(uv[0]), int(uv[1])), (int(ax[0]), int(ax[1]))


def prism_hull_host(uv, capacity=None):
    """Host-only rule C20, step 6 without the cap: the strict hull vertices of integer points (n, 2), counter-clockwise from the
    lexicographically smallest, as an (m, 2) int32 array."""
    lib = load_library()
    a = np.ascontiguousarray(uv, np.int32).reshape(-1, 2)
    cap = max(len(a), 1) if capacity is None else int(capacity)
    out = np.zeros((max(cap, 1), 2), np.int32)
    n = C.c_int()
    st = lib.cd_prism_hull_host(_ptr(a), len(a), _ptr(out), cap, C.byref(n))
    if st != CD_OK:
        raise CuboidError(st, "cd_prism_hull_host")
    return out[:n.value].copy()


def icp_plane_solve_host(sums, n):
    """Host-only rule C17, steps 3 and 4: (T float32 4x4, singular) from the 28 int64 sums of n correspondences."""
    lib = load_library()
    a = np.ascontiguousarray(sums, np.int64).reshape(28)
    T = np.zeros(16, np.float32)
    sg = C.c_int()
    st = lib.cd_icp_plane_solve_host(_ptr(a), int(n), _ptr(T), C.byref(sg))
    if st != CD_OK:
        raise CuboidError(st, "cd_icp_plane_solve_host")
    return T.reshape(4, 4), int(sg.value)


def icp_correspondence_threshold(d):
    """Host-only rule C8 conversion: (largest float32 f with float64(f) <= d*d, bounded flag); None = unbounded."""
    lib = load_library()
    f, b = C.c_float(), C.c_int()
    st = lib.cd_icp_correspondence_threshold(float("inf") if d is None else float(d), C.byref(f), C.byref(b))
    if st != CD_OK:
        raise CuboidError(st, "cd_icp_correspondence_threshold")
    return f.value, int(b.value)


def surface_guess(Rt):
    """Host-only rule C9: the ICP guess (4x4 float32, scene -> template) of a surface pose Rt (cd_surface_guess)."""
    lib = load_library()
    a = np.ascontiguousarray(Rt, np.float32).reshape(16)
    g = np.zeros(16, np.float32)
    f32 = C.POINTER(C.c_float)
    st = lib.cd_surface_guess(a.ctypes.data_as(f32), g.ctypes.data_as(f32))
    if st != CD_OK:
        raise CuboidError(st, "cd_surface_guess: non-finite input")
    return g.reshape(4, 4)


def shape_frame_host(xyz):
    """Host-only rule C13 steps 1-4 (cd_shape_frame_host): the CdShapeFrame of an (n, >= 3) float32 set; a refused or too small
    set is a record with its status, not an exception."""
    lib = load_library()
    a = np.asarray(xyz, np.float32)
    a = np.ascontiguousarray(a if a.ndim == 2 else a.reshape(-1, 3))
    r = CdShapeFrame()
    st = lib.cd_shape_frame_host(_ptr(a), a.shape[1] * 4, a.shape[0], C.byref(r))
    if st != r.status:
        raise CuboidError(st, "cd_shape_frame_host: bad arguments")
    return r


def shape_guess(cluster, template):
    """Host-only rule C13 step 5 (cd_shape_guess): (4x4 float32 scene -> template, flip 0..3 or -1 = identity fall-back)."""
    lib = load_library()
    g = np.zeros(16, np.float32)
    flip = C.c_int32()
    st = lib.cd_shape_guess(C.byref(cluster), C.byref(template), g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(flip))
    if st != CD_OK:
        raise CuboidError(st, "cd_shape_guess")
    return g.reshape(4, 4), int(flip.value)


def texture_project(cam, ccam, u, v, d):
    """Host-only rule C12 steps 1-6 for one pixel (cd_texture_project): (xyz float32[3], (iu, iv), textured)."""
    lib = load_library()
    xyz = np.zeros(3, np.float32)
    pix = np.zeros(2, np.int32)
    tex = C.c_int32()
    st = lib.cd_texture_project(C.byref(cam), C.byref(ccam), int(u), int(v), int(d), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                pix.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(tex))
    if st != CD_OK:
        raise CuboidError(st, "cd_texture_project: a camera the mapped calls refuse")
    return xyz, (int(pix[0]), int(pix[1])), int(tex.value)


def overlay_project(pose, params=None):
    """Host-only rule C11 steps 1-4 for one box (cd_overlay_project): (16 corner ints, drawn flag)."""
    lib = load_library()
    a = np.ascontiguousarray(pose, np.float64).reshape(16)
    box = CdOverlayBox()
    st = lib.cd_overlay_project(a.ctypes.data_as(C.POINTER(C.c_double)), None if params is None else C.byref(params), C.byref(box))
    if st != CD_OK:
        raise CuboidError(st, "cd_overlay_project: non-finite P, E or dims")
    return list(box.corners), int(box.drawn)


def verify_pixel(cam, pose, u, v, d, params=None):
    """Host-only rule C14 steps 2-4 for one pixel (cd_verify_pixel): (class CD_VERIFY_MISS .. CD_VERIFY_INVALID, z_r)."""
    lib = load_library()
    a = np.ascontiguousarray(pose, np.float64).reshape(16)
    cls, z = C.c_int32(-1), C.c_double(0.0)
    st = lib.cd_verify_pixel(C.byref(cam), a.ctypes.data_as(C.POINTER(C.c_double)), None if params is None else C.byref(params),
                             int(u), int(v), int(d), C.byref(cls), C.byref(z))
    if st != CD_OK:
        raise CuboidError(st, "cd_verify_pixel: bad camera, dims or tolerance")
    return cls.value, z.value


def verify_box_host(cam, depth, pose, params=None):
    """Host-only rule C14 for one box over one whole (H, W) uint16 image (cd_verify_box_host): a CdVerifyBox."""
    lib = load_library()
    depth = np.ascontiguousarray(depth, np.uint16)
    assert depth.shape == (cam.height, cam.width)
    a = np.ascontiguousarray(pose, np.float64).reshape(16)
    box = CdVerifyBox()
    st = lib.cd_verify_box_host(C.byref(cam), _ptr(depth), a.ctypes.data_as(C.POINTER(C.c_double)),
                                None if params is None else C.byref(params), C.byref(box))
    if st != CD_OK:
        raise CuboidError(st, "cd_verify_box_host: bad camera or parameters")
    return box


def verify_records(boxes, F=None, B=None):
    """An array of CdVerifyBox as a numpy array of verify.RECORD ((F, B) when both are given)."""
    from . import verify
    a = np.frombuffer(bytes(boxes), verify.RECORD)
    return a if F is None else a[:F * B].reshape(F, B)


def results_to_array(res):
    """View an array of CdFrameResult as a uint8 numpy array (F, FRAME_RESULT_BYTES)."""
    n = len(res)
    return np.frombuffer(res, dtype=np.uint8).reshape(n, FRAME_RESULT_BYTES)


def results_from_array(arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    n = arr.shape[0]
    out = (CdFrameResult * n)()
    C.memmove(out, arr.ctypes.data, n * FRAME_RESULT_BYTES)
    return out
