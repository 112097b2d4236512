/*
 * cuboid_hip.h - C-ABI of libcuboid_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-frame point-cloud path of dash-robotics/perception:
 *   crop -> voxel-downsample -> RANSAC ground plane -> extract -> Euclidean clusters ->
 *   point-to-point ICP of each cluster against a template cuboid.
 *
 * The reference has no FFI of its own for this path: every numeric step is a PCL object
 * used as "configure -> setInput -> one blocking compute call -> read outputs" inside the
 * ROS callbacks.  Each entry point below replaces one such PCL call site; the citation
 * next to it is the reference line it stands in for (paths relative to the reference
 * repository root; gps.cpp = cuboid_detection/src/ground_plane_segmentation.cpp,
 * icp.cpp = cuboid_detection/src/iterative_closest_point.cpp,
 * opd.cpp = object_detection/src/object_pose_detection.cpp).
 *
 * Conventions
 *  - plain pointers and sizes only; caller owns every buffer; capacities are passed in and
 *    counts are returned.  Point inputs are (base pointer, byte stride, count): x,y,z are
 *    float32 at byte offsets 0/4/8 of each record, so pcl::PointXYZ (16 B),
 *    pcl::PointXYZRGB (32 B) and raw sensor_msgs/PointCloud2 blobs pass without repacking.
 *  - every function returns CD_OK (0) or a negative cd_status; nothing throws or aborts
 *    across the boundary; cd_last_error() returns a message for the last failure.
 *  - a context is NOT thread-safe (mirrors the reference's single ros::spin() thread,
 *    gps.cpp:153); distinct contexts are independent (one per GPU / per process).
 *  - there is no CPU fallback: if no HIP device is usable cd_create() fails with
 *    CD_ERR_DEVICE and nothing else can be called.
 *  - results are a pure function of the inputs (the only randomness is PCL's fixed-seed
 *    RANSAC sampler, re-seeded per frame exactly as PCL does).
 */
#ifndef CUBOID_HIP_H
#define CUBOID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CD_ABI_VERSION 4
#define CD_MAX_TEMPLATES 8          /* template slots per context (BASELINE config 5 uses 5) */
#define CD_MAX_CLUSTERS_PER_FRAME 8 /* cluster slots in the fixed-size per-frame record; a frame with more clusters still
                                     * gets an ICP for every one of them (opd.cpp:376): see cd_get_cluster_results       */
#define CD_FRAME_MORE_CLUSTERS 1    /* cd_frame_result.flags: n_clusters > CD_MAX_CLUSTERS_PER_FRAME                    */
#define CD_FRAME_SURFACE_GUESS 2    /* cd_frame_result.flags: the frame's ICP started from its surface guess (CD_GUESS_SURFACE) */
#define CD_FRAME_CLUSTER_GUESS 4    /* cd_frame_result.flags: at least one cluster of the frame started from its rule-C13 guess (CD_GUESS_CLUSTER) */

typedef struct cd_context cd_context;

typedef enum cd_status {
    CD_OK = 0,
    CD_ERR_INVALID_ARG = -1,   /* null pointer, bad stride, count out of range             */
    CD_ERR_CAPACITY = -2,      /* input larger than the context / output buffer too small   */
    CD_ERR_DEVICE = -3,        /* HIP runtime error or no usable device                     */
    CD_ERR_NO_MODEL = -4,      /* RANSAC found no plane (PCL: empty inliers+coefficients)   */
    CD_ERR_FEW_CORRESPONDENCES = -5, /* ICP source has < 3 points, or (cd_icp with a maximum correspondence distance)
                                        an iteration kept < 3 correspondences (PCL: "Not enough correspondences") */
    CD_ERR_LEAF_TOO_SMALL = -6,/* voxel grid would overflow int32 indices (PCL warns)       */
    CD_ERR_NO_TEMPLATE = -7    /* template slot empty                                       */
} cd_status;

/* Parameters of the whole chain.  Defaults (cd_default_params) are the cuboid_detection
 * launch values with object_detection's clustering constants. */
typedef struct cd_params {
    /* S0 PassThrough "z" then "x" (gps.cpp:53-65, opd.cpp:273-289); limits inclusive, double */
    double crop_z_min, crop_z_max;      /* 0.0, 0.9  */
    double crop_x_min, crop_x_max;      /* -0.2, 0.2 */
    /* S1 VoxelGrid leaf (gps.cpp:72; launch: 0.005 cuboid / 0.001 object) */
    float leaf_size;
    int32_t rgb_offset;                 /* byte offset of packed rgb in a record, -1 = none */
    /* S2 SACSegmentation PLANE/RANSAC (gps.cpp:85-89) */
    double plane_distance_threshold;    /* launch: 0.015 */
    int32_t plane_max_iterations;       /* 1000 */
    int32_t plane_optimize;             /* setOptimizeCoefficients(true) */
    double plane_probability;           /* PCL default 0.99 */
    /* S3 ExtractIndices (gps.cpp:100): 1 keeps the non-plane points */
    int32_t extract_negative;
    /* S3b second PassThrough "z" on the extracted cloud (opd.cpp:331-336); 0 disables */
    int32_t crop2_enable;
    double crop2_z_min, crop2_z_max;    /* 0.0, 0.75 */
    /* S5 EuclideanClusterExtraction (opd.cpp:356-358); cluster_enable=0 feeds the whole
     * extracted cloud to ICP as one source (the cuboid_detection flavour, icp.cpp:156,171) */
    int32_t cluster_enable;
    int32_t cluster_min_size, cluster_max_size; /* 200, 25000 */
    double cluster_tolerance;           /* 0.02 */
    /* S6 IterativeClosestPoint (icp.cpp:173-176, opd.cpp:223-226) */
    int32_t icp_max_iterations;         /* 5000 */
    int32_t template_slot;              /* >= 0: that slot; -1: every loaded template, best fitness wins (BASELINE config 5) */
    double icp_transformation_epsilon;  /* 1e-9 */
    double icp_euclidean_fitness_epsilon; /* = icp_fitness_score param, 0.0004 (relative MSE) */
    double icp_accept_fitness;          /* acceptance test of icp.cpp:182, 0.0004 */
    /* Optional image-space gate of cuboid_detection/src/bbox_filter.cpp (within_bbox, :30-51): a point of
     * the extracted cloud is kept iff its projection u = (P0 x + P1 y + P2 z + P3)/w, v = ..., lies
     * strictly inside the rectangle (x1 < u < x2, y1 < v < y2).  P = CameraInfo.P (:60-62), row-major
     * 3x4 doubles; rectangle = the Rectangle message (:69-75).  0 disables (the launch default). */
    double bbox_P[12];
    int32_t bbox_enable;
    int32_t bbox_rect[4];               /* x1, y1, x2, y2 */
    /* Axis-constrained plane models of cuboid_detection/src/surface_normal_estimation.cpp:118-123
     * (seg.setModelType / setAxis / setEpsAngle): CD_PLANE = SACMODEL_PLANE (every other call site),
     * CD_PLANE_PERPENDICULAR = SACMODEL_PERPENDICULAR_PLANE (normal within eps of the axis),
     * CD_PLANE_PARALLEL = SACMODEL_PARALLEL_PLANE (normal within eps of perpendicular to the axis).
     * A hypothesis that violates the constraint scores 0 inliers but still counts as an iteration
     * (PCL: countWithinDistance starts with isModelValid); the refined model is tested again. */
    int32_t plane_model;
    float plane_axis[3];
    double plane_eps_angle;             /* radians; sne.cpp:123 uses 0.1 */
    /* Initial guess of the registration: pcl::Registration::align(output, guess).  The reference's live path calls
     * align(output) - the identity guess - and that is the default here (CD_GUESS_NONE).  Its authors meant to start from
     * the pose surface_normal_estimation publishes (icp.cpp:130-134 stores it, :165-167 moves the template by it; both
     * commented out / inert, and iterative_closest_point.launch:17-18 leaves the sne node out), so the guess is opt-in:
     * CD_GUESS_PARAMS uses icp_guess for every ICP of the call, CD_GUESS_PER_FRAME the matrix cd_set_frame_guesses stored
     * for the cluster's frame, CD_GUESS_SURFACE the guess the call derives from the frame's own surface fit (see
     * cd_surface_batch; fused calls only, cd_icp refuses it), CD_GUESS_CLUSTER the guess the call derives on the device for every
     * (cluster, template) pair from the cluster's own principal frame (rule C13, below; cd_icp accepts it: its source is the
     * cluster).  PCL semantics: the source is first moved by the guess (input_transformed = guess * source,
     * float32 4x4 * point), final_transformation_ starts as the guess, the iterations and the convergence tests run on the
     * moved cloud, getFinalTransformation() includes the guess and getFitnessScore() is that of final * source. */
    int32_t icp_use_guess;
    float icp_guess[16];                /* row-major, scene -> template */
} cd_params;

enum { CD_GUESS_NONE = 0, CD_GUESS_PARAMS = 1, CD_GUESS_PER_FRAME = 2, CD_GUESS_SURFACE = 3, CD_GUESS_CLUSTER = 4 };

enum { CD_PLANE = 0, CD_PLANE_PERPENDICULAR = 1, CD_PLANE_PARALLEL = 2 };

/* Output of cd_surface_frame: what surface_normal_estimation.cpp's callback (:167-234) derives from
 * three constrained plane fits.  Planes are in the callback's final order (most points first). */
typedef struct cd_surface_frame_result {
    float Rt[16];          /* row-major 4x4: columns normal[2], normal[1], normal[0], centroid (sne.cpp:218-222) */
    float coeff[3][4];     /* plane coefficients, sorted order                                  */
    float midpoint[3][4];  /* pcl::compute3DCentroid of each plane's points                      */
    int32_t n_points[3];   /* points of each plane                                               */
    int32_t iterations[3]; /* RANSAC iterations of the three fits, in FIT order                  */
    int32_t reserved[2];
} cd_surface_frame_result;

/* One ICP result: what icp.cpp:178-182 / opd.cpp:228-235 read back from PCL. */
typedef struct cd_cluster_result {
    int32_t size;          /* N_s, points in the cluster                              */
    int32_t iterations;    /* nr_iterations_                                          */
    int32_t converged;     /* icp.hasConverged()                                      */
    int32_t accepted;      /* converged && fitness < icp_accept_fitness (icp.cpp:182) */
    int32_t template_slot; /* slot this result was registered against (best fitness when all slots run) */
    int32_t reserved;
    float T[16];           /* getFinalTransformation(), row-major, scene -> template  */
    double fitness;        /* getFitnessScore()                                       */
    double pose[16];       /* T.cast<double>().inverse() (icp.cpp:179), row-major     */
} cd_cluster_result;

/* Fixed-size per-frame record (this is what is gathered across GPUs). */
typedef struct cd_frame_result {
    int32_t status;        /* cd_status of this frame                                 */
    int32_t n_cropped;     /* N_c after S0                                            */
    int32_t n_voxels;      /* N_v after S1                                            */
    int32_t n_plane;       /* refined plane inliers (S2)                              */
    int32_t n_objects;     /* N_o points after S3(+S3b)                               */
    int32_t n_clusters;    /* K clusters found (may exceed the slots below)           */
    int32_t ransac_iterations; /* PCL iterations_ consumed by the adaptive loop       */
    int32_t flags;         /* CD_FRAME_MORE_CLUSTERS                                  */
    float plane[4];        /* refined coefficients a,b,c,d                            */
    float pad[4];
    cd_cluster_result clusters[CD_MAX_CLUSTERS_PER_FRAME]; /* size-descending          */
} cd_frame_result;

void cd_default_params(cd_params* p);
int cd_abi_version(void);
/* sizeof() of the ABI structs, for FFI layers to verify their mirror of this header:
 * which = 0 cd_params, 1 cd_cluster_result, 2 cd_frame_result, 3 cd_timing, 4 cd_depth_camera, 5 cd_color_gate_params,
 * 6 cd_color_bbox, 7 cd_overlay_params, 8 cd_overlay_box. */
int cd_struct_size(int which);

/* Object lifetimes (replaces construction/destruction of the PCL objects and the node's
 * globals, icp.cpp:26-46).  max_points = largest N per frame, max_frames = largest batch. */
int cd_create(int device_id, int max_points, int max_frames, cd_context** out);
void cd_destroy(cd_context* ctx);
const char* cd_last_error(const cd_context* ctx);

/* pcl::io::loadPCDFile + icp.setInputTarget (icp.cpp:159,172; opd.cpp:398,222): the
 * template is uploaded once and stays device-resident. */
int cd_set_template(cd_context* ctx, int slot, const void* xyz, size_t stride_bytes, int m);

/* What cd_set_template found: the number of lattice faces of the slot's template, 0 when it is an arbitrary cloud (negative
 * cd_status on a bad slot).  cuboid_detection/templates/make_cuboid.py:38-55 writes every cuboid template as faces that are
 * Cartesian products of shared axis tables; cd_set_template verifies that structure bit by bit and, when it holds, the ICP
 * finds nearest neighbours in closed form instead of searching (same neighbour, same lowest-index tie rule). */
int cd_template_lattice_faces(const cd_context* ctx, int slot);

/* The correspondence search of icp.align on its own (pcl::registration::CorrespondenceEstimation -> KdTreeFLANN
 * nearestKSearch(k = 1), behind icp.cpp:178 / opd.cpp:228): for each of n query points the ORIGINAL index of the nearest
 * point of the slot's template (ties: lowest index) and the squared distance, float32, (dx*dx + dy*dy) + dz*dz.  Runs the
 * closed-form lattice search; CD_ERR_INVALID_ARG for a template that is not a lattice (its searches only exist inside the ICP
 * kernels). */
int cd_template_nearest(cd_context* ctx, int slot, const void* queries, size_t stride_bytes, int n, int32_t* out_index,
                        float* out_d2);

/* Diagnostic: ONE ICP iteration's state update on its own, for k records at once (no context; the current device).  The lattice
 * ICP finishes an iteration on a row of 16 lanes; this entry runs that code and the single-lane code every other ICP driver
 * uses side by side in one launch, four records per wave, and returns both results - they must be the same bytes.
 *   sums       k x 16 fixed-point moment sums (rule C4: [0..2] sum p, [3..5] sum q, [6..14] sum q_a p_b at 2^32, [15] sum d2 at 2^36)
 *   n          k correspondence counts
 *   states_in  k records of 152 bytes: float Tfinal[16], float T[16], double prev_mse, int32 iters, done, converged, status
 *   max_iter .. abs_mse  the convergence criteria (rot_thr = 1 - transformation epsilon as the library derives it)
 *   bounded    != 0: the variant with a maximum correspondence distance (fewer than three correspondences stop the ICP)
 *   states_row, states_lane  k outgoing records each;  done  k x 2 return values (row, single lane)
 *   unary      NULL, or 6 words: the row code's two short forms (square root of x in [1, +inf], reciprocal of 1 <= |x| < 2^126)
 *              compared with the IEEE operations for every float of those domains - [0] differing square roots, [1] the first
 *              such input's bits, [2], [3] the same for reciprocals, [4], [5] whether the library uses each short form */
int cd_icp_solve_batch(int k, const uint64_t* sums, const int32_t* n, const void* states_in, int max_iter, double trans_eps,
                       double rel_mse, double rot_thr, double abs_mse, int bounded, void* states_row, void* states_lane,
                       int32_t* done, uint64_t* unary);

/* Host-only (no context, no GPU): the lattice test of cd_set_template.  out (may be NULL) receives up to 8 faces x
 * {constant axis, fast axis, first index, points along the fast axis, points along the slow axis}.  Returns the number of
 * faces, 0 = not a lattice. */
int cd_lattice_detect(const void* xyz, size_t stride_bytes, int m, int32_t* out);

/* Host-only: does the lattice cd_lattice_detect finds have at most one face per constant axis (every three-face cuboid
 * template; not the six-face one)?  Such templates take the ICP's mask-free face code.  Returns 1 / 0 (0 also when the points
 * are no lattice).  out_axis_face[3] (may be NULL): the face whose constant axis is x / y / z, -1 = none; out_axis_c[3] (may be
 * NULL): that face's constant coordinate, NaN when none.  Both are all "none" when the result is 0. */
int cd_lattice_axes(const void* xyz, size_t stride_bytes, int m, int32_t* out_axis_face, float* out_axis_c);

/* S0+S1: two PassThrough filters + VoxelGrid::filter (gps.cpp:53-73).  out_xyz receives
 * N_v * 3 floats in ascending voxel-index order, out_rgb (may be NULL) N_v packed rgb. */
int cd_crop_voxel(cd_context* ctx, const void* points, size_t stride_bytes, int n,
                  const cd_params* prm, float* out_xyz, uint32_t* out_rgb, int capacity,
                  int* out_n_cropped, int* out_n_voxels);

/* One PassThrough filter as a call of its own: pcl::PassThrough<PCLPointCloud2>::filter (gps.cpp:53-58 "z", :61-65 "x";
 * opd.cpp:273-289, :331-336).  field = 0 / 1 / 2 for setFilterFieldName("x" / "y" / "z"), -1 for none (only non-finite points
 * go).  A record is kept iff x, y, z and the field are finite and !(v > limit_max || v < limit_min), v compared as double
 * (negative != 0, setFilterLimitsNegative: kept iff !(v < limit_max && v > limit_min)); kept records are copied whole
 * (stride_bytes each, a multiple of 4, >= 12) in their input order.  The fused calls (cd_crop_voxel, cd_ground_plane,
 * cd_process_*) apply the two crops of the launch files inside their first kernel; this entry is for a PassThrough that
 * stands alone. */
int cd_passthrough(cd_context* ctx, const void* points, size_t stride_bytes, int n, int field, double limit_min,
                   double limit_max, int negative, void* out_points, int capacity, int* out_n);

/* S2: seg.segment(*inliers, *coefficients) (gps.cpp:93).  inliers ascending.
 * The device draws the samples of a frame from 32768 precomputed random numbers and keeps PCL's shuffled index vector in a map of
 * 6144 usable slots; a sample that isSampleGood rejects (three collinear points with exactly equal float ratios: none on sensor
 * data) costs three numbers and up to three slots like one that is kept.  PCL has neither limit.  When PCL's loop would ask for a
 * hypothesis beyond them the call returns CD_ERR_CAPACITY (cd_last_error names the limits) instead of the best model so far;
 * cd_ground_plane does the same, a frame of a fused call carries CD_ERR_CAPACITY in its status - its record otherwise that of a
 * frame without a plane - while the call returns CD_OK, and the surface fits report the fit as failed (CD_ERR_NO_MODEL).  A
 * frame whose loop ends within what could be drawn is not affected. */
int cd_segment_plane(cd_context* ctx, const void* xyz, size_t stride_bytes, int n,
                     const cd_params* prm, float coeff[4], int32_t* inliers, int capacity,
                     int* out_n_inliers, int* out_iterations);

/* surface_normal_estimation.cpp:167-234, the whole callback: plane 0 = SACMODEL_PERPENDICULAR_PLANE to
 * `table_normal` (the plane parallel to the table top), planes 1,2 = SACMODEL_PARALLEL_PLANE, each fitted
 * (prm: distance threshold, iterations, optimize; eps 0.1 rad) on what the previous fit left over
 * (getNormal, :105-165; `invert` = the node's parameter of that name), then sorted by size, made
 * right-handed and assembled into the pose that the node broadcasts as estimated_cuboid_frame.
 * Returns CD_ERR_NO_MODEL when one of the three fits finds no plane (the reference reads an empty
 * coefficient vector there). */
int cd_surface_frame(cd_context* ctx, const void* xyz, size_t stride_bytes, int n, const float table_normal[3],
                     int invert, const cd_params* prm, cd_surface_frame_result* out);

/* cd_surface_frame over n_frames clouds in one call, every fit of every frame on the device: frame f is n_points[f] records
 * of `stride_bytes` (a multiple of 4, >= 12; x,y,z at 0/4/8) at xyz + f * points_per_frame * stride_bytes, its table normal
 * table_normals[3 f .. 3 f + 2].  out[f] and frame_status[f] (CD_OK / CD_ERR_NO_MODEL) are, byte for byte, what
 * cd_surface_frame returns for that cloud - a failed fit leaves iterations[] of the fits run so far and zeros elsewhere.
 * The call itself returns CD_OK unless an argument is bad (CD_ERR_INVALID_ARG), a cloud or the batch exceeds the context
 * (CD_ERR_CAPACITY) or the device fails.  The stage has FrameStates and point buffers of its own (allocated on first use). */
int cd_surface_batch(cd_context* ctx, const void* xyz, size_t stride_bytes, int points_per_frame, const int32_t* n_points,
                     int n_frames, const float* table_normals, int invert, const cd_params* prm, cd_surface_frame_result* out,
                     int32_t* frame_status);

/* Rule C9, host-only (no context, no GPU): the ICP guess of a surface pose.  Rt as sne publishes it ->
 * position t and quaternion q (cd_pose_to_position_quaternion) -> R(q) in double, q not normalised (poseMsgToEigen) -> of
 * R F, F = diag(1,1,1), diag(1,-1,-1), diag(-1,1,-1), diag(-1,-1,1), the first that turns the most template faces (outward
 * normals -x, -y, -z of make_cuboid.py's template) toward the camera -> guess = [R^T | -R^T t] rounded once to float32.  The
 * guess maps the scene to the template frame, so getFinalTransformation() includes it and the ICP pose stays the object's
 * pose in the camera frame (the reference's commented-out line moved the template by the pose instead: equal up to rounding
 * and the choice of F).  A non-finite Rt (or result): CD_ERR_INVALID_ARG. */
int cd_surface_guess(const float Rt[16], float guess[16]);

/* Principal frame of a point set and the per-cluster ICP guess (CD_GUESS_CLUSTER).  Canonical rule C13 (DESIGN.md §2;
 * perception_amd/cluster_frame.py restates it in plain Python and is its definition):
 *   a set is n float32 points.  status = CD_ERR_CAPACITY for n > 2^19, else CD_ERR_INVALID_ARG when a coordinate is not finite or
 *   |coordinate| > 64 (rule C4's range), else CD_ERR_FEW_CORRESPONDENCES for n < 3; such a record holds n, status and zeros.
 *   1. nine order-free sums by rule C4 (fixq(v, 32), int64) of x, y, z, xx, xy, xz, yy, yz, zz, every product one float32
 *      multiply; mean m_a = ((double)S_a 2^-32) / n, covariance c_ab = ((double)S_ab 2^-32) / n - m_a m_b, one double operation at
 *      a time;
 *   2. cyclic Jacobi on the 3x3 in double: 8 sweeps over the pairs (0,1), (0,2), (1,2), a rotation whose off-diagonal entry is
 *      exactly 0 skipped, + - x / sqrt only; eigenvalues descending (ties keep their order) = var, their vectors = the columns of
 *      axes; det < 0: the third column is negated;
 *   3. extents: q_a = ((A_0a dx + A_1a dy) + A_2a dz), d = (double)p - m; lo_a / hi_a = min / max over the set (a zero stored as +0);
 *   5. guess from a cluster record c and a template record t: sigma_a = sign(-(lo_t[a] + hi_t[a])), 0 when |lo_t[a] + hi_t[a]| <=
 *      2^-20 (hi_t[a] - lo_t[a]); w_a = -((A_c[0][a] m_c0 + A_c[1][a] m_c1) + A_c[2][a] m_c2); of F = diag(1,1,1), diag(1,-1,-1),
 *      diag(-1,1,-1), diag(-1,-1,1) the first with the strictly largest ((F_0 sigma_0) w_0 + (F_1 sigma_1) w_1) + (F_2 sigma_2) w_2;
 *      R = A_t F A_c^T, g = m_t - R m_c in double, left to right, each element rounded once to float32, last row 0 0 0 1.  A status
 *      != CD_OK on either side or a non-finite result: the identity.
 * G maps the scene to the template as rule C9's does: final_transformation_ starts as G, the sources are moved by G, pose stays the
 * object's pose in the camera frame. */
typedef struct cd_shape_frame {
    int32_t n, status;     /* points of the set; CD_OK or why there is no frame                      */
    double mean[3];
    double axes[9];        /* row-major 3x3, COLUMN a = principal axis a (largest variance first)    */
    double var[3];         /* variances along the axes, descending                                   */
    double lo[3], hi[3];   /* extents along the axes, relative to the mean                           */
} cd_shape_frame;
int cd_shape_frame_struct_size(void);   /* sizeof(cd_shape_frame) (cd_struct_size's list is closed) */

/* Host-only (no context, no GPU): rule C13 steps 1-4 for one set.  Returns out->status (the record is written whenever the
 * arguments are usable); a NULL pointer (xyz with n > 0, or out), n < 0 or a stride below 12: CD_ERR_INVALID_ARG, nothing written. */
int cd_shape_frame_host(const void* xyz, size_t stride_bytes, int n, cd_shape_frame* out);

/* The same for n_sets sets in ONE launch (k_shape.hip), from host points: set i is the records offsets[i] .. offsets[i + 1] - 1 of
 * xyz (offsets: n_sets + 1 ascending entries, offsets[0] >= 0), out[i] its record - byte for byte what cd_shape_frame_host gives.
 * A refused set is a result (its status), not a failure of the call.  The stage has buffers of its own (allocated on first use);
 * like every compute call it invalidates the read-backs of the last fused call. */
int cd_shape_frames(cd_context* ctx, const void* xyz, size_t stride_bytes, const int32_t* offsets, int n_sets, cd_shape_frame* out);

/* The record cd_set_template computed for the slot's template (host, at upload).  An empty slot: CD_ERR_NO_TEMPLATE. */
int cd_template_shape_frame(const cd_context* ctx, int slot, cd_shape_frame* out);

/* Host-only: rule C13 step 5.  guess receives the row-major 4x4, *flip (may be NULL) the index 0..3 of the chosen F, or -1 when
 * the guess is the identity fall-back (which is CD_OK).  NULL cluster / template_ / guess: CD_ERR_INVALID_ARG. */
int cd_shape_guess(const cd_shape_frame* cluster, const cd_shape_frame* template_, float guess[16], int32_t* flip);

/* The cluster records of the LAST fused call when it ran in CD_GUESS_CLUSTER mode: clusters [first, first + capacity) of `frame`
 * (rank order, as cd_get_cluster_results) into out.  Returns the number copied; CD_ERR_INVALID_ARG when that call was not in
 * the mode, or another compute call has run since.  They come back with the ICP stage's own result read-back: the mode adds no
 * synchronisation. */
int cd_get_cluster_shape_frames(const cd_context* ctx, int frame, int first, int capacity, cd_shape_frame* out);

/* sne's distance threshold for CD_GUESS_SURFACE (cd_params holds the ground plane's): context state like the correspondence
 * distance.  Default 0.015, the value of surface_normal_estimation.launch.  Not finite or <= 0: CD_ERR_INVALID_ARG, the
 * setting stays as it was. */
int cd_set_surface_distance_threshold(cd_context* ctx, double d);
int cd_get_surface_distance_threshold(const cd_context* ctx, double* out);

/* The per-frame surface results of the last fused call in CD_GUESS_SURFACE mode (what the sne node publishes: the pose and
 * the three coefficient messages): frames [first, first + capacity) into out / frame_status (either may be NULL).  Returns the
 * number copied, or CD_ERR_INVALID_ARG when the last fused call was not in surface mode or another compute call has run since
 * (the rule of cd_get_cluster_results).  A frame without a ground plane was not fitted: CD_ERR_NO_MODEL, a zero record. */
int cd_get_surface_results(const cd_context* ctx, int first, int capacity, cd_surface_frame_result* out, int32_t* frame_status);

/* S3 as a call of its own: pcl::ExtractIndices<PCLPointCloud2> (gps.cpp:96-101, opd.cpp:320-326; the fused calls extract
 * internally).  negative == 0: the records at `indices`, in the order of the list; negative != 0: the records whose index
 * is NOT in the list, in their original order (what both launch files use: setNegative(invert = true)).  Records are copied
 * whole - every field of the PointCloud2 blob - `stride_bytes` (a multiple of 4) each.  out_points holds `capacity` records. */
int cd_extract(cd_context* ctx, const void* points, size_t stride_bytes, int n, const int32_t* indices, int n_indices,
               int negative, void* out_points, int capacity, int* out_n);

/* bbox_filter: indices (ascending) of the points whose projection lies strictly inside the image
 * rectangle - cuboid_detection/src/bbox_filter.cpp:30-51 (within_bbox) and :84-103 (pcl_cb builds the
 * inlier list that its ExtractIndices keeps).  P = CameraInfo.P, row-major 3x4; rect = x1,y1,x2,y2.
 * The same test runs fused in cd_process_batch when cd_params.bbox_enable is set. */
int cd_bbox_filter(cd_context* ctx, const void* xyz, size_t stride, int n, const double P[12], const int32_t rect[4],
                   int32_t* out_indices, int capacity, int* out_n);

/* S5: ec.extract(cluster_indices) (opd.cpp:362).  labels[i] = cluster rank (0 = largest,
 * ties -> smaller first member index) or -1; sizes[k] for k < min(K, sizes_capacity). */
int cd_cluster(cd_context* ctx, const void* xyz, size_t stride_bytes, int n,
               const cd_params* prm, int32_t* labels, int32_t* sizes, int sizes_capacity,
               int* out_k);

/* S6: icp.align + getFinalTransformation + hasConverged + getFitnessScore
 * (icp.cpp:170-182).  aligned (may be NULL) receives n*3 floats.
 * With a maximum correspondence distance (cd_set_icp_max_correspondence_distance) an iteration that keeps fewer than 3
 * correspondences stops the ICP before its update, as PCL does: CD_ERR_FEW_CORRESPONDENCES, with out filled (T and
 * iterations as before that iteration, converged = accepted = 0, the fitness of T over all points) and aligned = T * source. */
int cd_icp(cd_context* ctx, int slot, const void* src_xyz, size_t stride_bytes, int n,
           const cd_params* prm, cd_cluster_result* out, float* aligned);

/* Whole chain, one call per batch: what opd.cpp:270-413 does per frame (this is what the
 * frames/s metric times).  `frames` holds n_frames * points_per_frame records.
 * plane_inliers / labels (may be NULL) receive per frame `points_per_frame` int32 slots:
 * the refined plane inlier indices (into the voxel cloud, ascending, -1 padded) and the
 * cluster label of every point of the extracted cloud (-1 padded). */
int cd_process_batch(cd_context* ctx, const void* frames, size_t stride_bytes,
                     int points_per_frame, int n_frames, const cd_params* prm,
                     cd_frame_result* results, int32_t* plane_inliers, int32_t* labels);

/* One frame: the body of the reference's callback / service handler (gps.cpp:43-112 followed by icp.cpp:150-182, or
 * opd.cpp:270-441) as one call - cd_process_batch with n_frames = 1 and `n` points. */
int cd_process_frame(cd_context* ctx, const void* points, size_t stride_bytes, int n, const cd_params* prm,
                     cd_frame_result* result, int32_t* plane_inliers, int32_t* labels);

/* opd.cpp:376-413 runs ICP on EVERY cluster of the frame and picks among all of them (:416-423).  The fixed-size record
 * carries the CD_MAX_CLUSTERS_PER_FRAME largest; when a frame has more (flags & CD_FRAME_MORE_CLUSTERS) the others - all of
 * them were registered as well - are read here.  Copies the results of clusters [first, first + capacity) of `frame`
 * (rank order: size descending) of the LAST cd_process_batch* call of this context into `out`; *out_total (may be NULL)
 * receives the number of clusters of that frame.  Returns the number of results copied, or a negative cd_status. */
int cd_get_cluster_results(const cd_context* ctx, int frame, int first, int capacity, cd_cluster_result* out,
                           int* out_total);

/* What the reference's nodes publish besides poses are CLOUDS of the frame they just processed; after a fused call those
 * are still resident on the device and are read back here (last cd_process_batch* / cd_process_frame call of this context;
 * any other compute call of the context invalidates them: CD_ERR_INVALID_ARG).
 *
 * cd_get_frame_cloud: which = CD_CLOUD_VOXELS, the VoxelGrid output (gps.cpp:73, opd.cpp:298); CD_CLOUD_OBJECTS, what is left
 * after the plane has been taken out (ExtractIndices, gps.cpp:96-101) and the second z crop - the cloud object_pose_detection
 * publishes on its <output> topic (opd.cpp:331-343).  Records are written in a PointCloud2 layout of the caller's choice:
 * `stride_bytes` (a multiple of 4, >= 12) per point, x,y,z float32 at byte offsets 0/4/8, the averaged packed colour at
 * rgb_offset (-1: none; a multiple of 4, >= 12), every other byte zero - with the INPUT's point_step and rgb offset this is
 * what fromPCL(ExtractIndices<PCLPointCloud2>(VoxelGrid<PCLPointCloud2>(input))) hands to the publisher. */
enum { CD_CLOUD_VOXELS = 0, CD_CLOUD_OBJECTS = 1 };
int cd_get_frame_cloud(cd_context* ctx, int frame, int which, void* out_records, size_t stride_bytes, int rgb_offset,
                       int capacity, int* out_n);

/* The points of cluster k (rank order, as in cd_get_cluster_results) of `frame`: aligned == 0 the cluster as extracted
 * (ExtractIndices of opd.cpp:378-387), aligned != 0 the cloud icp.align(output) returned for it (opd.cpp:228, the cloud
 * behind /icp/registered_pcl, opd.cpp:259-262; icp.cpp:178,193 -> /icp/aligned_points).  Records of `stride_bytes`
 * (multiple of 4, >= 12): x,y,z at 0/4/8; with stride_bytes >= 16 the fourth word is 1.0f, which is what pcl::PointXYZ holds
 * there and pcl::toROSMsg(PointCloud<PointXYZ>) puts on the wire (point_step 16); further bytes zero.
 * (When several templates were matched in separate passes and the best one was not the last, the aligned cloud is
 * final_transformation * cluster evaluated once, not the iterated cloud - equal up to float32 rounding.) */
int cd_get_cluster_points(cd_context* ctx, int frame, int k, int aligned, void* out_points, size_t stride_bytes,
                          int capacity, int* out_n);

/* The body of ground_plane_segmentation's callback (gps.cpp:43-112) as ONE call: two PassThrough filters, VoxelGrid,
 * SACSegmentation, ExtractIndices - one upload of the PointCloud2 blob, one download of the cloud to publish.
 * out_records receives the kept voxels in the INPUT's record layout (stride_bytes per record, centroid at 0/4/8, averaged
 * colour at prm->rgb_offset, other bytes zero), *out_n their number, coeff the refined plane, *out_n_inliers the size of
 * the refined inlier set.  prm->crop2_enable / bbox_enable apply as in the fused chain (the gps node sets both 0).
 * When RANSAC finds no plane the status is CD_ERR_NO_MODEL, coeff is untouched and the records are what PCL's
 * ExtractIndices yields for an empty index list (negative: every voxel; otherwise none), as gps.cpp:93-107 publishes. */
int cd_ground_plane(cd_context* ctx, const void* points, size_t stride_bytes, int n, const cd_params* prm, float coeff[4],
                    void* out_records, int capacity, int* out_n, int* out_n_inliers);

/* Per-frame initial guesses for cd_params.icp_use_guess == CD_GUESS_PER_FRAME: n_frames row-major 4x4 float32 matrices
 * (scene -> template), frame f of the following cd_process_batch* calls uses guesses[16 f .. 16 f + 15] for each of its
 * clusters (the granularity of the reference: one sne pose per frame, icp.cpp:130-134).  n_frames = 0 clears them. */
int cd_set_frame_guesses(cd_context* ctx, const float* guesses, int n_frames);

/* CD_GUESS_SURFACE (cd_process_batch[_device], cd_process_frame, cd_process_depth_batch[_device]): after S3 every frame with a
 * ground plane runs cd_surface_batch's fits on its objects cloud (the CD_CLOUD_OBJECTS read-back), table normal = its own
 * plane[0..2], invert = 1, threshold = cd_set_surface_distance_threshold, the other plane parameters as prm; rule C9 turns
 * each pose into the frame's guess (identity where the fit fails), and the ICP runs as CD_GUESS_PER_FRAME would with those
 * guesses; frames whose guess came from the fit get CD_FRAME_SURFACE_GUESS.  The guesses cd_set_frame_guesses stored are
 * untouched.  One guess per FRAME, as in the reference: meaningful when a frame holds one object (the cuboid_detection
 * scenario) - with several boxes the fits run across them (their coplanar tops all go to the first fit). */

/* IterativeClosestPoint::setMaxCorrespondenceDistance (the line icp.cpp:175 / opd.cpp:225 leave commented out): context
 * state that applies to every ICP of the following cd_icp, cd_process_frame, cd_process_batch[_device] and
 * cd_process_depth_batch[_device] calls on ctx.  Default: unbounded.  Rule C8: source point i keeps its
 * correspondence iff (double)d2_i <= max_distance * max_distance (the boundary is kept), d2_i being the float32 squared
 * distance to its nearest template point (the search itself is unchanged); only kept correspondences enter the
 * transformation estimate and the MSE of the convergence test; fewer than 3 stop the ICP before that iteration's update
 * (converged = accepted = 0, T and iterations as they were; in a batch that is a result, the frame's status stays CD_OK).
 * getFitnessScore is unchanged: all points, unbounded.  +inf, and any distance whose square is >= FLT_MAX (PCL's default
 * sqrt(DBL_MAX) among them), is unbounded: the default path, byte for byte.  Negative or NaN: CD_ERR_INVALID_ARG, the
 * setting stays as it was. */
int cd_set_icp_max_correspondence_distance(cd_context* ctx, double max_distance);
int cd_get_icp_max_correspondence_distance(const cd_context* ctx, double* out);

/* Host-only (no context, no GPU): rule C8's conversion.  *out_d2_max = the largest float32 f with (double)f <= d * d
 * (what the kernels compare d2 against), *out_bounded = 0 when d * d >= FLT_MAX (nothing is ever rejected), else 1.
 * Either pointer may be NULL.  Negative or NaN d: CD_ERR_INVALID_ARG. */
int cd_icp_correspondence_threshold(double max_distance, float* out_d2_max, int* out_bounded);

/* Same, input already resident in device memory (HBM) of the context's GPU.  A context works on its own
 * non-blocking HIP stream: there is no implicit ordering against the NULL stream or any other stream, so the
 * caller must have completed its writes to d_frames (e.g. hipStreamSynchronize on the producing stream)
 * before the call.  The call itself is synchronous: results are final when it returns. */
int cd_process_batch_device(cd_context* ctx, const void* d_frames, size_t stride_bytes,
                            int points_per_frame, int n_frames, const cd_params* prm,
                            cd_frame_result* results, int32_t* plane_inliers,
                            int32_t* labels);

/* Depth-image input: what the D435 produces before its driver builds /camera/depth/color/points on the CPU, deprojected on
 * the device (depth_image_proc-style, from sensor_msgs/Image + CameraInfo).  Depth is 16UC1 with tightly packed rows
 * (step == 2 * width); the optional colour is rgb8 registered pixel for pixel to the depth (step == 3 * width).  Pixel (u, v)
 * becomes record v * width + u of an ORGANIZED cloud of 16-byte records x, y, z float32 + packed rgb, by canonical rule C7
 * (float32, no contraction, IEEE '/'):
 *     z = (float)d * depth_scale,  x = (((float)u - cx) / fx) * z,  y = (((float)v - cy) / fy) * z,
 *     rgb word = (r << 16) | (g << 8) | b (0 without colour);
 *     d == 0 is invalid: x = y = z = quiet NaN (0x7FC00000), the rgb word as for a valid pixel.
 * A batch of F frames is F images back to back (depth: F * width * height uint16, colour: F * width * height * 3 bytes).
 * Bad input (null depth, width * height 0 or over max_points, n_frames out of 1 .. max_frames, an unknown colour mode, colour
 * requested with a NULL pointer, fx / fy / depth_scale not finite or <= 0) is CD_ERR_INVALID_ARG before anything is copied
 * or launched. */
enum { CD_COLOR_NONE = 0, CD_COLOR_RGB8 = 1 };
typedef struct cd_depth_camera {      /* sensor_msgs/CameraInfo of the depth stream; int32/float only, no padding holes */
    int32_t width, height;            /* width*height <= the context's max_points */
    float fx, fy, cx, cy;             /* K[0], K[4], K[2], K[5]; plumb_bob with D == 0 only */
    float depth_scale;                /* metres per unit (D435: 0.001) */
    int32_t color;                    /* CD_COLOR_NONE | CD_COLOR_RGB8 */
} cd_depth_camera;

/* The D435 depth stream of the reference's README.md:74-78: 640 x 480, K of its CameraInfo, 1 mm per unit, no colour. */
void cd_default_depth_camera(cd_depth_camera* cam);

/* One frame, host in and host out: the organized cloud (width * height records, NaN where the depth is 0) that a node
 * publishes for the image, in a PointCloud2 layout of the caller's choice - `stride_bytes` (a multiple of 4, >= 12) per
 * record, x,y,z at 0/4/8, the rgb word at rgb_offset (-1: none; a multiple of 4, >= 12), every other byte zero.  `capacity`
 * records fit in out_records; *out_n receives width * height (also when the capacity is too small: CD_ERR_CAPACITY). */
int cd_depth_to_cloud(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color,
                      void* out_records, size_t stride_bytes, int rgb_offset, int capacity, int* out_n);

/* Whole chain on n_frames depth images: exactly cd_process_batch on the canonical organized clouds - stride 16,
 * points_per_frame = width * height, rgb_offset 12 with colour and -1 without (prm->rgb_offset is IGNORED).  Results,
 * cd_get_cluster_results / cd_get_frame_cloud / cd_get_cluster_points and cd_get_timing (the deprojection counts in
 * stage [0]) are those of that call.  The images are uploaded into buffers of their own (one copy each, on the context's
 * stream) and deprojected on the device. */
int cd_process_depth_batch(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color,
                           int n_frames, const cd_params* prm, cd_frame_result* results, int32_t* plane_inliers,
                           int32_t* labels);

/* Same, images already resident in device memory of the context's GPU (ordering as cd_process_batch_device: the caller has
 * completed its writes before the call). */
int cd_process_depth_batch_device(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* d_depth, const uint8_t* d_color,
                                  int n_frames, const cd_params* prm, cd_frame_result* results, int32_t* plane_inliers,
                                  int32_t* labels);

/* Unregistered image pair: what the D435 delivers when its driver does NOT align the streams - raw 16UC1 depth at the depth
 * camera's size and K, raw rgb8 colour at the COLOUR camera's size and K (README.md:48-54 of the reference: 640 x 480 both,
 * fx 384.09 against 616.82) and the depth -> colour extrinsics (the topic draw_bbox.py subscribes to).  The mapped calls build the
 * cloud the driver publishes as /camera/depth/color/points - points in the DEPTH camera's frame, each coloured by the colour
 * pixel it projects to - on the device.  Canonical rule C12 (float32, one IEEE operation at a time, no
 * contraction), for pixel (u, v) of depth frame f with depth value d:
 *   1. d == 0: x = y = z = quiet NaN (0x7FC00000), rgb word 0 (rule C7 gives such a pixel its own colour; here there is no point
 *      to project);
 *   2. x, y, z by rule C7 from the depth camera's fx, fy, cx, cy, depth_scale;
 *   3. Xc = ((R[0] x + R[1] y) + R[2] z) + t[0], Yc from R[3..5], t[1], Zc from R[6..8], t[2]: p_colour = R p_depth + t, R
 *      row-major - the mapping of cd_overlay_params.E (the RealSense Extrinsics message stores its rotation COLUMN-major: a
 *      caller transposes it);
 *   4. pu = (Xc / Zc) * fx_c + cx_c, pv = (Yc / Zc) * fy_c + cy_c; iu = floor(pu + 0.5f), iv = floor(pv + 0.5f) (pixel centres at
 *      integer coordinates, as in C7);
 *   5. the point is TEXTURED iff Zc > 0, pu and pv are finite and 0 <= iu < width_c, 0 <= iv < height_c; its rgb word is
 *      (r << 16) | (g << 8) | b of colour pixel (iu, iv) of frame f's colour image;
 *   6. an untextured point: CD_NOTEX_DROP (default; the driver with allow_no_texture_points off) x = y = z = quiet NaN, rgb 0 -
 *      the crop removes it like any invalid pixel; CD_NOTEX_KEEP: xyz kept, rgb 0;
 *   7. there is NO occlusion test: a depth point hidden from the colour camera takes the colour of whatever the colour camera
 *      sees in that direction (the driver has none either).
 * Parity with librealsense is UNPINNED, as for PCL and OpenCV: perception_amd/texture_map.py restates the rule on the CPU and the
 * device equals it byte for byte.  Lens distortion (D == 0 only), aligning the depth image TO the colour geometry (the scatter
 * direction), occlusion handling and bgr8 / 32FC1 encodings are out of scope. */
enum { CD_NOTEX_DROP = 0, CD_NOTEX_KEEP = 1 };
typedef struct cd_color_camera {      /* 80 bytes, int32/float only, no padding holes */
    int32_t width, height;            /* of the colour image; width*height <= the context's max_points */
    float fx, fy, cx, cy;             /* K of /camera/color/camera_info; plumb_bob with D == 0 only */
    float R[9], t[3];                 /* depth -> colour: p_colour = R p_depth + t, R row-major, t in metres */
    int32_t no_texture;               /* CD_NOTEX_DROP | CD_NOTEX_KEEP */
    int32_t reserved;
} cd_color_camera;

/* 640 x 480, the colour K of the reference's README.md:52, R = identity, t = 0 (the reference records no extrinsic values),
 * CD_NOTEX_DROP. */
void cd_default_color_camera(cd_color_camera* ccam);
int cd_color_camera_struct_size(void);   /* sizeof(cd_color_camera) (cd_struct_size's list is closed) */

/* Host-only (no context, no GPU): steps 1-6 for ONE pixel.  xyz = the record's x, y, z; pix = (iu, iv), or (-1, -1) when the
 * point is not textured; *textured = 0 / 1.  Any output pointer may be NULL.  cam->color is not looked at.  A NULL camera, or one
 * the mapped calls refuse (below), is CD_ERR_INVALID_ARG. */
int cd_texture_project(const cd_depth_camera* cam, const cd_color_camera* ccam, int u, int v, uint16_t d, float xyz[3],
                       int32_t pix[2], int32_t* textured);

/* cd_depth_to_cloud under rule C12: `color` is ONE ccam->width x ccam->height rgb8 image, tightly packed.
 * The mapped calls refuse, with CD_ERR_INVALID_ARG before anything is copied or launched: everything cd_depth_to_cloud /
 * cd_process_depth_batch refuse; a NULL ccam or colour pointer; cam->color != CD_COLOR_RGB8; ccam->width * ccam->height 0 or over
 * max_points; ccam->fx or fy not finite or <= 0; a non-finite cx, cy, R or t; an unknown no_texture. */
int cd_depth_to_cloud_mapped(cd_context* ctx, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* depth,
                             const uint8_t* color, void* out_records, size_t stride_bytes, int rgb_offset, int capacity, int* out_n);

/* Whole chain on n_frames unregistered pairs: exactly cd_process_batch on the rule-C12 clouds - stride 16, points_per_frame =
 * cam->width * cam->height, rgb_offset 12 (prm->rgb_offset is IGNORED).  Depth: n_frames images of cam->width x cam->height
 * uint16 back to back; colour: n_frames images of ccam->width x ccam->height x 3 bytes back to back, independent of the depth
 * size.  Results, read-backs and cd_get_timing (the mapping counts in stage [0]) are those of that call.
 * CD_BBOX_COLOR: rule C10 runs on the batch's RAW colour images at ccam->width x ccam->height, so its rectangles (and
 * cd_get_frame_bboxes) are in COLOUR pixels, where object_detection.py finds them.  The gate (bbox_filter.cpp) multiplies the
 * depth-frame points by prm->bbox_P as it is: the reference passes the colour camera's P there and so ignores the extrinsics; a
 * caller who wants them honoured passes P_colour x E (3x4 times 4x4, E as in cd_overlay_params).
 * cd_draw_last_results[_device] after a mapped call takes the ccam->width x ccam->height colour images, with params->P the colour
 * camera's and params->E the extrinsics. */
int cd_process_depth_batch_mapped(cd_context* ctx, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* depth,
                                  const uint8_t* color, int n_frames, const cd_params* prm, cd_frame_result* results,
                                  int32_t* plane_inliers, int32_t* labels);
/* Same, images already resident in device memory of the context's GPU (ordering as cd_process_batch_device). */
int cd_process_depth_batch_mapped_device(cd_context* ctx, const cd_depth_camera* cam, const cd_color_camera* ccam,
                                         const uint16_t* d_depth, const uint8_t* d_color, int n_frames, const cd_params* prm,
                                         cd_frame_result* results, int32_t* plane_inliers, int32_t* labels);

/* Colour gate: the node that PRODUCES the rectangle of the bbox gate, cuboid_detection/scripts/object_detection.py:25-62
 * (/camera/color/image_raw -> /object_detection/bbox), for every image of a batch on the device.  Canonical rule C10
 * (DESIGN.md §2), integers only, on rgb8 (the script's bgr8 conversion only swaps channels):
 *   1. 8-bit HSV, H in 0..179 (cvtColor BGR2HSV): v = max, diff = v - min, s = (diff * sdiv[v] + 2048) >> 12,
 *      h0 = (v == r) ? g - b : (v == g) ? b - r + 2 diff : r - g + 4 diff, h = (h0 * hdiv[diff] + 2048) >> 12 (arithmetic),
 *      h += 180 if h < 0; sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)) in double, half to even, 0 at 0;
 *   2. mask = (h <= h_lo_max || h >= h_hi_min) && s >= s_min && v >= v_min (the script's two inRange calls, or-ed);
 *   3. opening: one 9x9 erosion (outside the image counts as set) then one 9x9 dilation (outside counts as clear) - erode and
 *      dilate with 5x5 ones, iterations = 2; the script's threshold(200) on a 0/255 image is the identity;
 *   4. 8-connected components (image border pixels are ordinary pixels); each component's outer border followed through pixel
 *      centres (Suzuki-Abe, from the component's first raster pixel); area2 = |shoelace sum| = 2 * contourArea.  Hole borders,
 *      which RETR_LIST also returns, enclose strictly less than their component's outer border and never win;
 *   5. the component with the largest area2; ties: the one whose first raster pixel comes first;
 *   6. rect = (x - margin, y - margin, x + w + margin, y + h + margin) of its pixel bounds x, y, w, h - NOT clipped to the image;
 *   7. no component: found = 0, rect = (0, 0, 0, 0), which keeps no point (the script publishes nothing and bbox_filter.cpp:23
 *      keeps its zero-initialised rectangle).  Frames of a batch are independent.
 * Parity with a real OpenCV build is UNPINNED (OpenCV is not a dependency here, like PCL): the semantics are OpenCV 3.x's 8-bit
 * paths as the rule states them; perception_amd/color_gate.py restates the rule on the CPU and the device equals it bit for bit. */
typedef struct cd_color_gate_params {   /* rule C10; int32 only */
    int32_t h_lo_max, h_hi_min;         /* 10, 175: H in 0 .. h_lo_max or h_hi_min .. 179 */
    int32_t s_min, v_min;               /* 50, 100 (upper bounds 255)                     */
    int32_t margin;                     /* 10                                             */
    int32_t reserved[3];
} cd_color_gate_params;
typedef struct cd_color_bbox {
    int32_t rect[4];                    /* x1, y1, x2, y2 as the Rectangle message        */
    int32_t found;                      /* 0: no component (rect all zero)                */
    int32_t area2;                      /* 2 * contourArea of the chosen component        */
    int32_t n_components;
    int32_t n_mask;                     /* set pixels after the opening                   */
} cd_color_bbox;
void cd_default_color_gate_params(cd_color_gate_params* g);

/* Rule C10 on n_frames tightly packed rgb8 images (width * height * 3 bytes each, back to back): out[f] for every frame.
 * params == NULL: the defaults.  Null pointers, width * height 0 or over max_points, n_frames outside 1 .. max_frames, H bounds
 * outside 0..179, S / V minima outside 0..255 or a negative margin: CD_ERR_INVALID_ARG before any copy or launch.
 * CD_ERR_CAPACITY: a border walk ran past its step bound (8 * width * height: cannot happen on a healthy device); no
 * rectangle of that call is to be used. */
int cd_color_bbox_batch(cd_context* ctx, const uint8_t* rgb8, int width, int height, int n_frames,
                        const cd_color_gate_params* params, cd_color_bbox* out);
/* Same, images already resident in device memory of the context's GPU (ordering as cd_process_batch_device). */
int cd_color_bbox_batch_device(cd_context* ctx, const uint8_t* d_rgb8, int width, int height, int n_frames,
                               const cd_color_gate_params* params, cd_color_bbox* out);

/* Where the gate of the fused calls (cd_params.bbox_enable != 0) takes its rectangle from; bbox_P always comes from cd_params.
 *   CD_BBOX_PARAMS (default): cd_params.bbox_rect, one rectangle for the whole call.
 *   CD_BBOX_PER_FRAME: frame f of cd_process_batch[_device], cd_process_depth_batch[_device] and cd_process_frame is gated by
 *     rects[4 f .. 4 f + 3] of cd_set_frame_bboxes (like cd_set_frame_guesses; n_frames = 0 clears them).  Fewer stored
 *     rectangles than frames: CD_ERR_INVALID_ARG before anything is launched.
 *   CD_BBOX_COLOR: cd_process_depth_batch[_device] with CD_COLOR_RGB8 and cd_process_depth_batch_mapped[_device] only - rule C10
 *     runs on the batch's colour images before
 *     the extraction and its rectangles feed the gate on the device (no host round trip).  Every other fused entry point, or a
 *     depth call without colour: CD_ERR_INVALID_ARG.  `params` (NULL = defaults) are the rule's parameters.
 * With bbox_enable == 0 the source does not matter; cd_bbox_filter, cd_extract, cd_ground_plane and cd_surface_* ignore it.
 * An unknown source or bad params: CD_ERR_INVALID_ARG, the setting stays as it was.
 * cd_get_frame_bboxes: the rectangles the gate of the LAST fused call used, frames [first, first + capacity) (CD_BBOX_COLOR: the
 * full records; CD_BBOX_PER_FRAME: the stored rectangle, found = 1, the other fields 0).  Returns the number copied, or
 * CD_ERR_INVALID_ARG when that call's gate was off or read cd_params, or another compute call has run since. */
enum { CD_BBOX_PARAMS = 0, CD_BBOX_PER_FRAME = 1, CD_BBOX_COLOR = 2 };
int cd_set_frame_bboxes(cd_context* ctx, const int32_t* rects, int n_frames);
int cd_set_bbox_source(cd_context* ctx, int source, const cd_color_gate_params* params);
int cd_get_bbox_source(const cd_context* ctx, int* source);
int cd_get_frame_bboxes(const cd_context* ctx, int first, int capacity, cd_color_bbox* out);

/* Overlay: the one consumer of the chain's poses that the reference has, cuboid_detection/scripts/draw_bbox.py:44-83 (the eight
 * /icp/bbox_points corners projected with CameraInfo.P x the depth->colour extrinsics, 12 green lines of thickness 2 over the
 * colour image), for every image of a batch on the device.  Canonical rule C11, per box = a row-major double pose
 * (cd_cluster_result.pose) and the dimensions dims = l, w, h:
 *   1. corners = cd_bbox_corners(pose, l, w, h): float32, the order of icp.cpp:99-106; each widened to double;
 *   2. M = P E in double, every entry ((p0 e0 + p1 e1) + p2 e2) + p3 e3, no contraction;
 *   3. h_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3]; u = h_0 / h_2, v = h_1 / h_2 (IEEE divide); pixel = truncation
 *      toward zero (astype('int'), draw_bbox.py:62);
 *   4. a box is SKIPPED (drawn = 0, corners reported as zeros) when any corner has a non-finite u or v, h_2 <= 0 or a pixel
 *      coordinate of magnitude over 8192.  h_2 <= 0 is a deviation: the script would draw the mirrored box of a point behind
 *      the camera;
 *   5. edges: the 12 corner pairs of draw_bbox.py:66-77 - 01 02 04 13 15 23 26 37 45 46 57 67;
 *   6. pixel p of the image is painted for the edge with integer end points a, b iff, with d = b - a, e = p - a, L = d.d,
 *      s = e.d (int64):  (L == 0 or s <= 0) and 4 e.e <= t^2;  or  s >= L and 4 |p - b|^2 <= t^2;  or otherwise
 *      4 (e x d)^2 <= t^2 L - every pixel within t / 2 of the segment, round caps, integers only;
 *   7. painted pixels receive rgb; every other byte of the image is unchanged; nothing outside the image is touched.  All boxes
 *      of a call share one colour, so the order of drawing cannot matter; frames are independent.
 * Parity with a real OpenCV build's cv2.line (its fixed-point thick-line polygon) is UNPINNED, as for rule C10:
 * perception_amd/overlay.py restates the rule on the CPU and the device equals it byte for byte. */
typedef struct cd_overlay_params {      /* no padding holes */
    double P[12];                       /* CameraInfo.P of the colour stream, row-major 3x4                       */
    double E[16];                       /* depth -> colour extrinsics, row-major 4x4; identity for registered images */
    double dims[3];                     /* l, w, h of every box of the call (iterative_closest_point.launch:39-41) */
    int32_t thickness;                  /* 1 .. 64; draw_bbox.py: 2                                                */
    uint8_t rgb[3];                     /* r, g, b written to painted pixels; draw_bbox.py: 0, 255, 0              */
    uint8_t pad;
    int32_t reserved[6];
} cd_overlay_params;
typedef struct cd_overlay_box {
    int32_t corners[16];                /* u0, v0, ... u7, v7 (step 3); all zero when drawn == 0                   */
    int32_t drawn;                      /* 0: skipped (step 4), or no box in this slot                             */
    int32_t reserved[3];
} cd_overlay_box;
/* D435 P of the reference's README.md:78 (the K of cd_default_depth_camera, zero fourth column), E = identity, dims 0.2 / 0.1 /
 * 0.03, thickness 2, green. */
void cd_default_overlay_params(cd_overlay_params* p);

/* Host-only (no context, no GPU): steps 1-4 for one box.  params == NULL: the defaults.  A skipped box is a result (CD_OK,
 * drawn = 0); NULL pose / out, or a non-finite P, E or dims: CD_ERR_INVALID_ARG. */
int cd_overlay_project(const double pose[16], const cd_overlay_params* params, cd_overlay_box* out);

/* Rule C11 on n_frames tightly packed rgb8 images (width * height * 3 bytes each, back to back), drawn IN PLACE.  Frame f has
 * n_boxes[f] <= boxes_per_frame boxes; the pose of its box b is poses[(f * boxes_per_frame + b) * 16 .. + 15]; out receives
 * n_frames * boxes_per_frame records in the same order (slots at and beyond n_boxes[f]: all zero).  params == NULL: the defaults.
 * Checked before any copy or launch, CD_ERR_INVALID_ARG: a null rgb8 / poses / n_boxes / out, width * height 0 or over
 * max_points, width or height over 8192, n_frames outside 1 .. max_frames, boxes_per_frame outside 1 .. 1024, thickness outside
 * 1 .. 64, a non-finite P, E or dims, a negative n_boxes[f] or one over boxes_per_frame.  A non-finite pose is no error: that
 * box is skipped.  The host form uploads the images, draws and downloads them again.  Like every compute call
 * these two invalidate the read-backs of the last fused call (cd_draw_last_results does not). */
int cd_draw_boxes_batch(cd_context* ctx, uint8_t* rgb8, int width, int height, int n_frames, const double* poses,
                        const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* params, cd_overlay_box* out);
/* Same, images already resident in device memory of the context's GPU (ordering as cd_process_batch_device; the images are
 * final when the call returns).  poses, n_boxes and out are host memory. */
int cd_draw_boxes_batch_device(cd_context* ctx, uint8_t* d_rgb8, int width, int height, int n_frames, const double* poses,
                               const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* params, cd_overlay_box* out);

/* The poses of the LAST fused call of the context (cd_process_batch[_device], cd_process_frame, cd_process_depth_batch[_device])
 * drawn into that call's n_frames images - e.g. the CD_COLOR_RGB8 images of cd_process_depth_batch_device, still resident.
 * boxes_per_frame is CD_MAX_CLUSTERS_PER_FRAME: slot k of frame f is clusters[k] of its record; which = CD_DRAW_ACCEPTED draws
 * the slots with accepted != 0, CD_DRAW_ALL every slot below min(n_clusters, CD_MAX_CLUSTERS_PER_FRAME); the other slots of
 * `out` (n_frames * CD_MAX_CLUSTERS_PER_FRAME records) are zero.  Every box has params->dims.  The validity rule of
 * cd_get_cluster_results: CD_ERR_INVALID_ARG when there is no such call or another compute call has run since; the draw calls
 * themselves leave the fused call's read-backs as they are (both `which` can be drawn in turn).  Only the poses go to the
 * device; in the _device form the images never visit the host.  Argument checks as cd_draw_boxes_batch. */
enum { CD_DRAW_ACCEPTED = 0, CD_DRAW_ALL = 1 };
int cd_draw_last_results(cd_context* ctx, uint8_t* rgb8, int width, int height, int which, const cd_overlay_params* params,
                         cd_overlay_box* out);
int cd_draw_last_results_device(cd_context* ctx, uint8_t* d_rgb8, int width, int height, int which, const cd_overlay_params* params,
                                cd_overlay_box* out);

/* Pose verification: the cuboid of a pose rendered into the 16UC1 depth image the pose was found in, and every pixel it covers
 * compared with what the sensor measured there - a machine-readable verdict beside `converged && fitness < accept`
 * (icp.cpp:182), which accepts poses whose box the sensor saw straight through.  Canonical rule C14.  All
 * arithmetic is double, one IEEE operation at a time, no contraction, IEEE '/'.  Per box: the row-major double pose [R t; 0 0 0 1]
 * (box to camera, cd_cluster_result.pose), dims = l, w, h, the cd_depth_camera of the image (fx, fy, cx, cy, depth_scale
 * widened from float32 to double) and the tolerance tau:
 *   1. SKIP: the box is not verified (verified = 0, every count 0) when any of the 12 entries of R, t is non-finite, or any of
 *      the 8 corners (sx, sy, sz in +-1) has zc = ((R[2][0] (sx l/2) + R[2][1] (sy w/2)) + R[2][2] (sz h/2)) + t[2] with !(zc > 0):
 *      a box not wholly in front of the camera is not rendered;
 *   2. ray of pixel (u, v): dx = ((double)u - cx) / fx, dy = ((double)v - cy) / fy, direction (dx, dy, 1); for each box axis a:
 *      o_a = -((R[0][a] t[0] + R[1][a] t[1]) + R[2][a] t[2]),  dd_a = (R[0][a] dx + R[1][a] dy) + R[2][a],  half_a = dims[a] / 2;
 *   3. slabs, written as comparisons so that a NaN behaves the same everywhere: tn = -inf, tf = +inf, miss = false; an axis with
 *      dd_a == 0: miss |= fabs(o_a) > half_a and nothing else; any other axis: t1 = (-half_a - o_a) / dd_a, t2 = (half_a - o_a) /
 *      dd_a, lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1, tn = lo > tn ? lo : tn, tf = hi < tf ? hi : tf.  The pixel is HIT
 *      iff !miss && tn <= tf && tn > 0; the rendered depth is z_r = tn, the camera z of the entry point (a camera inside the box
 *      hits nothing);
 *   4. class of a hit pixel with depth value d, z_m = (double)d * depth_scale: INVALID if d == 0; THROUGH if z_m - z_r > tau (the
 *      sensor saw past where the box should be); OCCLUDED if z_r - z_m > tau (something nearer: neutral); AGREE otherwise (both
 *      boundaries are AGREE);
 *   5. record: the int32 counts n_hit, n_agree, n_through, n_occluded, n_invalid; agree_abs_um = the sum over AGREE pixels of
 *      (int64)(fabs(z_m - z_r) * 1e6 + 0.5) (an integer sum: its order cannot matter; a term of 2^63 or more counts as
 *      2^63 - 1); score = n_agree / (double)(n_agree + n_through), 0.0 when that sum is 0; passed = verified && n_agree >=
 *      min_agree && score >= min_score;
 *   6. the counts are defined over every pixel of the image (the device skips pixels outside a rectangle around the projected
 *      corners that it can prove are misses); boxes and frames are independent of each other - boxes do not occlude one another;
 *      nothing is written to the depth image.
 * The 180-degree flips of a cuboid are the same solid and therefore give the same record: what a grasp wants.
 * perception_amd/verify.py restates the rule on the CPU over whole images and the device equals it in every field. */
typedef struct cd_verify_params {       /* no padding holes */
    double dims[3];                     /* l, w, h of every box (defaults 0.2, 0.1, 0.03)                           */
    double slot_dims[CD_MAX_TEMPLATES][3]; /* cd_verify_last_results with use_slot_dims: dims of the record's template_slot */
    double tolerance;                   /* tau, metres; default 0.01; finite, >= 0                                  */
    double min_score;                   /* default 0.9; finite                                                      */
    int32_t min_agree;                  /* default 200 (the cluster minimum); >= 0                                  */
    int32_t use_slot_dims;              /* 0 / 1                                                                    */
    int32_t reserved[6];
} cd_verify_params;
typedef struct cd_verify_box {
    int32_t verified, passed, n_hit, n_agree, n_through, n_occluded, n_invalid, reserved;
    int64_t agree_abs_um;
    double score;
} cd_verify_box;                        /* 48 bytes; all zero for an empty slot */
enum { CD_VERIFY_ACCEPTED = 0, CD_VERIFY_ALL = 1 };
enum { CD_VERIFY_MISS = 0, CD_VERIFY_AGREE = 1, CD_VERIFY_THROUGH = 2, CD_VERIFY_OCCLUDED = 3, CD_VERIFY_INVALID = 4 };
/* dims 0.2 / 0.1 / 0.03 (also in every slot_dims row), tolerance 0.01, min_score 0.9, min_agree 200, use_slot_dims 0. */
void cd_default_verify_params(cd_verify_params* p);
/* sizeof as this library was built: which = 0 cd_verify_params, 1 cd_verify_box, anything else -1. */
int cd_verify_struct_size(int which);

/* Host-only (no context, no GPU): steps 2-4 for pixel (u, v) with depth value d of a box with params->dims.  *cls receives
 * CD_VERIFY_MISS .. CD_VERIFY_INVALID, *z_r the rendered depth when the pixel is hit (0.0 otherwise).  Step 1 is not applied.
 * params == NULL: the defaults.  NULL cam / pose / cls / z_r, fx / fy / depth_scale not finite or <= 0, an unknown colour mode, a
 * non-finite or negative dims or tolerance: CD_ERR_INVALID_ARG. */
int cd_verify_pixel(const cd_depth_camera* cam, const double pose[16], const cd_verify_params* params, int u, int v, uint16_t d,
                    int32_t* cls, double* z_r);
/* Host-only: the whole rule for one box over one cam->width x cam->height image, every pixel of it.  Checks as cd_verify_pixel,
 * plus a NULL depth / out, width or height < 1, a non-finite min_score and a negative min_agree. */
int cd_verify_box_host(const cd_depth_camera* cam, const uint16_t* depth, const double pose[16], const cd_verify_params* params,
                       cd_verify_box* out);

/* Rule C14 on n_frames tightly packed 16UC1 images (cam->width * cam->height uint16 each, back to back; no colour image is read).
 * Layout as cd_draw_boxes_batch: frame f has n_boxes[f] <= boxes_per_frame boxes, the pose of its box b is
 * poses[(f * boxes_per_frame + b) * 16 .. + 15], out receives n_frames * boxes_per_frame records in the same order (slots at
 * and beyond n_boxes[f]: all zero).  box_dims == NULL: every box has params->dims; otherwise the box in slot (f, b) has
 * box_dims[(f * boxes_per_frame + b) * 3 .. + 2].  params == NULL: the defaults.  Checked before any copy or launch,
 * CD_ERR_INVALID_ARG: a null cam / depth / poses / n_boxes / out, the camera fields cd_process_depth_batch refuses (fx, fy or
 * depth_scale not finite or <= 0, an unknown colour mode), width * height 0 or over max_points, n_frames outside 1 .. max_frames, boxes_per_frame outside 1 .. 1024,
 * a non-finite or negative dims, box_dims (of an existing box) or tolerance, a non-finite min_score, a negative min_agree, a
 * negative n_boxes[f] or one over boxes_per_frame.  A non-finite pose is no error: that box has verified = 0.  The host form
 * uploads the images into a buffer that nothing else uses; in the _device form only poses, dims and the records cross the bus.
 * Like every compute call these two invalidate the read-backs of the last fused call (cd_verify_last_results does not). */
int cd_verify_boxes_batch(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, const double* poses,
                          const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* params,
                          cd_verify_box* out);
/* Same, images already resident in device memory of the context's GPU (ordering as cd_process_batch_device).  poses, n_boxes,
 * box_dims and out are host memory. */
int cd_verify_boxes_batch_device(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* d_depth, int n_frames, const double* poses,
                                 const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* params,
                                 cd_verify_box* out);

/* The poses of the LAST fused call of the context verified against that call's n_frames depth images: the image that was
 * deprojected for cd_process_depth_batch[_device]; the RAW depth image for cd_process_depth_batch_mapped[_device] (its poses are
 * in the depth camera's frame); the caller's depth image of the same frame for the cloud-fed calls.  Slots, `which`
 * (CD_VERIFY_ACCEPTED / CD_VERIFY_ALL), validity rule and effect on the read-backs exactly as cd_draw_last_results: out holds
 * n_frames * CD_MAX_CLUSTERS_PER_FRAME records, slot k of frame f is clusters[k]; a slot that is not selected is all zero; the
 * fused call's records and read-backs, and a later cd_draw_last_results, stay as they were.  Every box has params->dims, or -
 * use_slot_dims != 0 - params->slot_dims[template_slot of its record] (then every row of slot_dims is checked like dims).
 * Argument checks as cd_verify_boxes_batch. */
int cd_verify_last_results(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* depth, int which, const cd_verify_params* params,
                           cd_verify_box* out);
int cd_verify_last_results_device(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* d_depth, int which,
                                  const cd_verify_params* params, cd_verify_box* out);

/* Point labels: for every INPUT record (pixel) of the last fused call of the context, what the chain made of it.  Canonical rule
 * C15; the rule is by provenance - a point takes the class of the voxel VoxelGrid put it in, and the voxel's class
 * is read off the call's own plane_inliers, object cloud and labels, so a label can never disagree with the call's records.
 * One uint8 per record:
 *   CD_LABEL_INVALID  x, y or z is not finite (a depth value of 0 under rule C7);
 *   CD_LABEL_CROPPED  finite, but outside the S0 limits (the z limits, then the x limits; double limits, inclusive);
 *   CD_LABEL_PLANE    kept by S0, its voxel is in the call's refined inlier list and not in its object cloud;
 *   CD_LABEL_OBJECT   its voxel is in the object cloud with cluster label -1 or a cluster rank >= 248;
 *   CD_LABEL_GATED    kept by S0, its voxel is in neither set (removed by S3b or the bbox gate; a non-inlier with
 *                     extract_negative = 0; the frame's status ended the chain before S3);
 *   5 .. 7            reserved, never written;
 *   CD_LABEL_CLUSTER0 + r   its voxel is in the object cloud with cluster label r, 0 <= r < 248 (the rank order of
 *                     cd_get_cluster_results; with cluster_enable = 0 every object voxel has rank 0).
 * A point's voxel is the cell floor(p * inv_leaf) - min_b in float32, inv_leaf = 1.0f / leaf; a voxel's number is the rank of its
 * idx = i + j dx + k dx dy among the frame's occupied cells: the order of CD_CLOUD_VOXELS.  perception_amd/point_labels.py
 * restates the rule in numpy and the device equals it byte for byte. */
enum { CD_LABEL_INVALID = 0, CD_LABEL_CROPPED = 1, CD_LABEL_PLANE = 2, CD_LABEL_OBJECT = 3, CD_LABEL_GATED = 4, CD_LABEL_CLUSTER0 = 8 };
/* The caller passes the frames of the fused call AGAIN (as cd_verify_last_results takes the depth images again: the library does
 * not keep its input).  out receives n_frames * points_per_frame bytes in record order - for an organized cloud it is the label
 * image.  CD_ERR_INVALID_ARG: a null pointer; no fused call, or another compute call has run since (the validity rule of
 * cd_get_cluster_results); n_frames, points_per_frame or stride_bytes differing from that call's (a depth-fed call has 16-byte
 * records).  Data that is not that call's input has a defined result: the rule evaluated on that data against the call's grid -
 * a cell that holds no voxel reads CD_LABEL_GATED, and a cell outside the grid is a miss that is never used as an index.
 * The fused call's records and read-backs stay valid, and draw, verify and label calls can follow each other in any order.
 * _device: frames and out are device memory of the context's GPU (ordering as cd_process_batch_device). */
int cd_label_points_last(cd_context* ctx, const void* frames, size_t stride_bytes, int points_per_frame, int n_frames, uint8_t* out);
int cd_label_points_last_device(cd_context* ctx, const void* d_frames, size_t stride_bytes, int points_per_frame, int n_frames,
                                uint8_t* d_out);
/* The same from the n_frames tightly packed 16UC1 depth images of the call, deprojected by rule C7 (no colour image is read):
 * out is the label image, cam->width * cam->height bytes per frame.  Serves cd_process_depth_batch[_device], a cloud-fed call
 * whose records were the rule-C7 cloud of these images, and cd_process_depth_batch_mapped[_device] with CD_NOTEX_KEEP.  A
 * mapped call with CD_NOTEX_DROP is REFUSED with CD_ERR_INVALID_ARG: rule C12 gives its untextured pixels NaN coordinates, which
 * rule C7 does not, so the depth image alone does not say what that call's records were - label such a call through
 * cd_label_points_last with the records of cd_depth_to_cloud_mapped.  Further CD_ERR_INVALID_ARG: a null pointer, fx, fy or
 * depth_scale not finite or <= 0, width * height or n_frames differing from that call's. */
int cd_label_depth_last(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, uint8_t* out);
int cd_label_depth_last_device(cd_context* ctx, const cd_depth_camera* cam, const uint16_t* d_depth, int n_frames, uint8_t* d_out);

/* Tint: labels drawn over tightly packed rgb8 images in place.  For each pixel and channel c' = (c (255 - a) + p a + 127) / 255
 * in integers, (p, a) = palette->rgba[label][channel], [3].  palette == NULL: the default palette - alpha 0 for CD_LABEL_INVALID
 * and CD_LABEL_CROPPED (the pixel stays as it is), a grey for the plane, orange for CD_LABEL_OBJECT, a dark red for
 * CD_LABEL_GATED, and eight cluster colours that repeat with the rank.  A host-side utility of the image domain: it reads no
 * state of a fused call and invalidates none.  CD_ERR_INVALID_ARG: a null image or labels, width * height 0 or over max_points,
 * n_frames outside 1 .. max_frames. */
typedef struct cd_label_palette { uint8_t rgba[256][4]; } cd_label_palette;
void cd_default_label_palette(cd_label_palette* palette);
/* sizeof as this library was built: which = 0 cd_label_palette, anything else -1 (cd_struct_size's list is closed). */
int cd_label_struct_size(int which);
int cd_tint_labels_batch(cd_context* ctx, uint8_t* rgb8, const uint8_t* labels, int width, int height, int n_frames,
                         const cd_label_palette* palette);
int cd_tint_labels_batch_device(cd_context* ctx, uint8_t* d_rgb8, const uint8_t* d_labels, int width, int height, int n_frames,
                                const cd_label_palette* palette);

/* Statistical outlier removal on the object cloud (pcl::StatisticalOutlierRemoval in front of EuclideanClusterExtraction).
 * Canonical rule C16; perception_amd/outlier_filter.py restates it in numpy and the device equals it bit for
 * bit - every dist_i, the statistics and the kept set.  Parity with a real PCL is unpinned, as for every other rule (its k-d
 * tree's order among equidistant neighbours and its summation order are its own).  For a cloud of n points, mean_k in
 * 1 .. CD_OUTLIER_MAX_MEAN_K, std_mul and negative:
 *   1. points with a non-finite coordinate are dropped first: never a neighbour, not counted, never in the output; m finite points;
 *   2. m <= mean_k: every finite point is kept (negative or not), nothing is computed, the statistics are reported as 0;
 *   3. for finite point i the float32 squared distances (dx*dx + dy*dy) + dz*dz to ALL finite points, itself included; of these
 *      the mean_k + 1 smallest as a multiset less exactly one, the smallest (itself; a coincident twin's 0 stays and counts);
 *   4. their float32 square roots added into a double in ascending order; dist_i = (float)(sum / mean_k);
 *   5. over the finite points in cloud order, sequentially in double: sum += d, sq += d * d; mean = sum / m,
 *      var = (sq - sum * sum / m) / (m - 1), stddev = sqrt(var), threshold = mean + std_mul * stddev;
 *   6. kept iff (double)dist_i <= threshold (negative: iff not); the output keeps the cloud's order.
 *
 * cd_set_outlier_filter: context state, as the ICP correspondence distance is.  mean_k = 0 turns the filter off (the default:
 * no kernel of the fused calls changes and every output is byte for byte what it was); otherwise 1 <= mean_k <= 63 and std_mul
 * finite, else CD_ERR_INVALID_ARG and the setting stays.  With the filter on, every fused call (cd_process_batch[_device],
 * cd_process_frame, cd_process_depth_batch[_device], cd_process_depth_batch_mapped[_device]) filters each frame's object cloud
 * between S3 and S5, and everything behind it takes the filtered cloud: clustering, the surface and cluster guesses, ICP,
 * n_objects of the frame record, the `labels` output, cd_get_frame_cloud(CD_CLOUD_OBJECTS) (whole records: the colour travels
 * with the point) and cd_get_cluster_points.  The label calls (rule C15) give a voxel that S3 moved into the object cloud and
 * the filter removed CD_LABEL_GATED.  cd_ground_plane, cd_cluster, cd_icp and every other call of a single stage are unaffected.
 * CD_OUTLIER_LDS_TILE: the candidates the kernel stages in LDS at a time (the sizes around it are where its loop turns). */
#define CD_OUTLIER_MAX_MEAN_K 63
#define CD_OUTLIER_LDS_TILE 1024
int cd_set_outlier_filter(cd_context* ctx, int mean_k, double std_mul, int negative);
int cd_get_outlier_filter(const cd_context* ctx, int* mean_k, double* std_mul, int* negative);
/* What the filter did to `frame` of the last fused call: the object points before it, how many it removed, and the statistics
 * of step 5 (0 when step 2 applied).  Any pointer may be NULL.  CD_ERR_INVALID_ARG when that call ran without the filter, has
 * been invalidated (the validity rule of cd_get_cluster_results) or had no such frame. */
int cd_get_outlier_stats(const cd_context* ctx, int frame, int* n_before, int* n_removed, double* mean, double* stddev,
                         double* threshold);
/* The filter as a call of its own (pcl::StatisticalOutlierRemoval::filter(indices)): the kept indices ascending, like
 * cd_bbox_filter.  out_dist (may be NULL) receives n floats, dist_i, 0 for a dropped non-finite point; stats (may be NULL)
 * mean, stddev, threshold.  Out-of-range arguments (mean_k outside 1 .. 63, a non-finite std_mul, n < 0, a stride below 12 or
 * no multiple of 4, a null pointer) give CD_ERR_INVALID_ARG before anything is launched; n above the context's max_points
 * CD_ERR_CAPACITY; capacity < kept CD_ERR_CAPACITY with *out_n = kept.  The context's own setting is neither read nor
 * changed; like every compute call it invalidates the read-backs of the last fused call. */
int cd_outlier_filter(cd_context* ctx, const void* xyz, size_t stride_bytes, int n, int mean_k, double std_mul, int negative,
                      int32_t* out_indices, int capacity, int* out_n, float* out_dist, double stats[3]);

/* Plane-weighted ICP for lattice templates: an opt-in transformation estimate, off by default.  Canonical rule C17 (DESIGN.md
 * §2); perception_amd/icp_plane.py restates it in numpy and the device equals it bit for bit.  It is NOT
 * pcl::registration::TransformationEstimationPointToPlaneLLS: that estimator is the case lambda = 0 below, which is singular
 * whenever a cluster touches two faces only; parity with any PCL estimator is neither claimed nor pinned.
 * Within an iteration, in getFitnessScore(), `accepted` and the records it is the library's ICP: correspondences by rule C5
 * (bounded by C8), step, X <- T X, Tfinal <- T Tfinal, DefaultConvergenceCriteria in its order.  Only the step differs.
 * State of a (cluster, template) pair: X, Tfinal, prev_mse, iters and `latched`, initially true iff switch_distance is +inf.
 *   1. q, d2 and q's face come from rule C5; n = the correspondences kept (C8); n < 3 stops the ICP as under C8.  w = the
 *      constant axis of q's face (a lattice face's normal is a coordinate axis).
 *   2. lambda_it = latched ? (float)tangent_weight : 1.0f.  For each axis a with b, c the next two cyclically:
 *      r = q_a - s_a, g = (a == w) ? 1.0f : lambda_it, u = g s_c, v = g s_b, h = g r; the nine terms of the axis are
 *      g, u, v, u s_c, v s_b, u s_b, h, h s_c, h s_b - single float32 operations, no FMA.  The 27 terms and d2 go into 64-bit
 *      integer sums by rule C4 (2^32; 2^36 for d2): nothing depends on how points are divided among lanes, waves or passes.
 *   3. In double, on the sums divided by their scale, unknowns (omega_x, omega_y, omega_z, t_x, t_y, t_z); component a's row has
 *      +s_c at omega_b, -s_b at omega_c, 1 at t_a.  Axis a (x, y, z in turn) adds S3 to M[ob][ob], S4 to M[oc][oc], -S5 to
 *      M[ob][oc], S1 to M[ob][ta], -S2 to M[oc][ta], S0 to M[ta][ta], and S7, -S8, S6 to the right-hand side at ob, oc, ta.
 *      M = L D L^T (the lower Cholesky factorisation without its square roots), column by column, inner sums ascending, every
 *      operation rounded; column j is singular iff !(d_j > M_jj * 2^-40).  A singular solve stops the ICP before the update,
 *      as too few correspondences do: converged = accepted = 0, T = identity, Tfinal and iterations as they were.  Forward
 *      substitution ascending, back substitution descending (the module's docstring has every association).
 *   4. R = the rotation of the quaternion (1, omega / 2): with k = omega / 2 and m = ((1 + kx^2) + ky^2) + kz^2, each entry its
 *      polynomial divided by m in double (R00 = (((1 + kx^2) - ky^2) - kz^2) / m, R01 = (2 (kx ky - kz)) / m, ...), cast to
 *      float32, as is t.  No sqrt, no library function.
 *   5. mse = sum d2 / n; latched |= (mse <= switch_distance^2), in double, after the solve of every iteration that reaches it
 *      (a one-way latch: a switch that can reopen cycles).  Then icp_step's tail unchanged.
 *
 * cd_set_icp_plane_weight: context state, as the correspondence distance is; applies to every ICP of the following cd_icp and
 * fused calls.  tangent_weight == 0 turns the mode off (the default: every record, launch and kernel is what it was);
 * otherwise tangent_weight in [1/1024, 1] and switch_distance >= 0 or +inf (plane weights from the first iteration).  Anything
 * else, NaN included: CD_ERR_INVALID_ARG and the setting stays.  CD_ICP_PLANE_WEIGHT_DEFAULT / CD_ICP_PLANE_SWITCH_DEFAULT are
 * the recommended pair (a switch at 0.02 m is too early, weights from 0.55 m away diverge: INTEGRATION.md §3).
 * With the mode on every live cluster goes to the mode's own driver (k_icp_plane); CUBOID_ICP_LATTICE / CUBOID_ICP_MODE do not
 * apply and no generic driver implements it.  A call that would use a loaded template that is not a lattice
 * (cd_template_lattice_faces == 0) returns CD_ERR_INVALID_ARG before anything is launched.  In cd_icp a singular stop returns
 * CD_ERR_FEW_CORRESPONDENCES (the message says "singular") with out filled; in a batch it is a result, the frame stays CD_OK. */
#define CD_ICP_PLANE_WEIGHT_DEFAULT (1.0 / 32.0)
#define CD_ICP_PLANE_SWITCH_DEFAULT 0.01
#define CD_ICP_PLANE_WEIGHT_MIN (1.0 / 1024.0)
typedef struct cd_icp_plane_stats {
    int32_t plane_iterations;        /* iterations run with `latched` true                      */
    int32_t first_plane_iteration;   /* the first of them, 1-based; 0: never latched            */
    int32_t stopped_singular;        /* 1: the ICP stopped on a singular step                   */
    int32_t reserved;
} cd_icp_plane_stats;
int cd_set_icp_plane_weight(cd_context* ctx, double tangent_weight, double switch_distance);
int cd_get_icp_plane_weight(const cd_context* ctx, double* tangent_weight, double* switch_distance);
/* Indexed like cd_get_cluster_results (the stats of the template whose result the cluster kept); after a stand-alone cd_icp
 * the result is at frame 0, index 0.  Returns the number copied; CD_ERR_INVALID_ARG when the call ran with the mode off, has
 * been invalidated by another compute call, or had no such frame. */
int cd_get_cluster_plane_stats(const cd_context* ctx, int frame, int first, int count, cd_icp_plane_stats* out);
/* Host only (no context, no GPU): steps 3 and 4 on the 28 sums of n correspondences (sum 9 a + j: term j of axis a; sum 27:
 * d2, unused here).  T row-major; *singular = 1 and T = identity for a singular system or n < 1. */
int cd_icp_plane_solve_host(const int64_t sums[28], int n, float T[16], int32_t* singular);

/* Coarse-to-fine ICP: an opt-in resolution pyramid of two levels, off by default.  Canonical rule C18;
 * perception_amd/icp_coarse.py is the rule in numpy.  It changes results: the fine level starts from another pose than the
 * call's guess, so it may end in another minimum (INTEGRATION.md §3 has what was measured).
 * Context state (stride s, min_points m); s = 0 is off.  With s >= 2 a (cluster, template) pair whose cluster has n >= m points
 * is eligible:
 *   1. the coarse set is the points p[j s], j = 0 .. ceil(n / s) - 1, of the cluster in extraction order (the order of
 *      cd_get_cluster_points(aligned = 0); in cd_icp the order of src_xyz);
 *   2. the coarse ICP is the ICP this library runs on that set as a cluster of its own: same template, cd_params, rule C8 / C17
 *      setting and guess mode (CD_GUESS_CLUSTER computes rule C13 on the coarse set).  Its result is T_c;
 *   3. the fine ICP is the ICP of the whole cluster started from T_c, as CD_GUESS_PARAMS with icp_guess = T_c runs it;
 *      icp_max_iterations applies to each level on its own.  Every record of the cluster (T, pose, iterations, converged,
 *      fitness, accepted, aligned cloud, plane stats) is the fine level's;
 *   4. a coarse ICP that stopped (fewer than three correspondences under rule C8, a singular step of rule C17) or whose T_c has
 *      a non-finite entry is dropped: the fine level starts from the call's own guess, as with the mode off.
 * Pairs that are not eligible run as with the mode off.  With CD_GUESS_CLUSTER the shape records
 * (cd_get_cluster_shape_frames, CD_FRAME_CLUSTER_GUESS) stay those of the whole cluster.
 *
 * cd_set_icp_coarse: applies to every ICP of the following cd_icp and fused calls.  stride 0 (min_points is ignored and kept as
 * it was) or 2 .. 64 with min_points >= 3 * stride; anything else CD_ERR_INVALID_ARG and the setting stays.  Turning the mode on
 * grows the context's ICP source buffers, and the object-cloud buffer the outlier filter swaps with one of them, by two thirds
 * (the coarse sets lie behind a stage's clusters, so they fit any stage of the context); CD_ERR_DEVICE when
 * that allocation fails; the call that grows them invalidates the read-backs of the last fused call, as a compute call does. */
typedef struct cd_icp_coarse_stats {
    int32_t n_coarse;            /* points of the coarse set; 0: the pair was not eligible                          */
    int32_t coarse_iterations;
    int32_t coarse_converged;
    int32_t coarse_status;       /* CD_OK, or CD_ERR_FEW_CORRESPONDENCES for a coarse ICP that stopped              */
    double coarse_fitness;       /* getFitnessScore of the coarse set under T_c                                     */
    int32_t used;                /* 0 not eligible, 1 the fine level started from T_c, 2 it fell back (step 4)      */
    int32_t reserved;
} cd_icp_coarse_stats;
#define CD_ICP_COARSE_STRIDE_MAX 64
int cd_set_icp_coarse(cd_context* ctx, int stride, int min_points);
int cd_get_icp_coarse(const cd_context* ctx, int* stride, int* min_points);
int cd_icp_coarse_struct_size(void);   /* sizeof(cd_icp_coarse_stats) (cd_struct_size's list is closed) */
/* Host only (no context, no GPU): step 1's indices of a set of n points.  Returns their count, 0 when the set is not eligible
 * or the setting is not one cd_set_icp_coarse takes; out_indices (may be NULL) is written only when the count fits capacity. */
int cd_icp_coarse_subsample(int n, int stride, int min_points, int32_t* out_indices, int capacity);
/* Indexed like cd_get_cluster_results (the stats of the template whose result the cluster kept); after a stand-alone cd_icp
 * the result is at frame 0, index 0.  Returns the number copied; CD_ERR_INVALID_ARG when the call ran with the mode off, has
 * been invalidated by another compute call, or had no such frame. */
int cd_get_cluster_coarse_stats(const cd_context* ctx, int frame, int first, int count, cd_icp_coarse_stats* out);

/* Median-distance correspondence rejection inside the ICP: opt-in, off by default.  Canonical rule C19;
 * perception_amd/icp_reject.py is the rule in numpy and the device equals it bit for bit.  It restates
 * pcl::registration::CorrespondenceRejectorMedianDistance as added by IterativeClosestPoint::addCorrespondenceRejector
 * (nth_element at size / 2 over the squared distances, keep <= median * factor, after the correspondence estimation's own
 * bound); parity with a real PCL is unpinned.  It changes results: the step is estimated from fewer correspondences.
 * With a factor f set, every ICP iteration takes its correspondences by rule C5; rule C8's bound leaves the set K0 (every point
 * when it bounds nothing).  Then
 *   1. |K0| < 3 stops the ICP as rule C8 does (T = identity, converged = 0, Tfinal and iterations as they were);
 *   2. m = the float32 d2 of rank floor(|K0| / 2) (0-based, ascending) over K0: the upper median, nothing averaged;
 *   3. thr = (double) m * f, one rounded double product;
 *   4. a correspondence of K0 is kept iff (double) d2 <= thr;
 *   5. fewer than three kept: the stop of step 1;
 *   6. the 16 moment sums of rule C4, the MSE of the convergence tests and the solve's n are over the kept ones only.
 * X <- T X moves every point, getFitnessScore() is over all points and unbounded, `accepted`, the pose and the order of the
 * convergence tests are untouched.
 *
 * cd_set_icp_median_rejection: context state, as the correspondence distance is; applies to every ICP of the following cd_icp and
 * fused calls, the coarse level of rule C18 included.  factor == 0 turns the mode off (the default: every record, launch and
 * kernel is what it was); otherwise a finite factor > 0.  NaN, a negative value or an infinity: CD_ERR_INVALID_ARG and the
 * setting stays.  With the mode on every live cluster goes to the mode's own driver (the sliced loop with k_icp_reject behind
 * every iteration); CUBOID_ICP_LATTICE / CUBOID_ICP_MODE do not apply.  Together with plane-weighted ICP (rule C17) every ICP
 * entry point returns CD_ERR_INVALID_ARG before anything is launched.  In cd_icp a stop returns CD_ERR_FEW_CORRESPONDENCES with
 * out filled, as under rule C8; in a batch it is a result, the frame stays CD_OK. */
typedef struct cd_icp_reject_stats {
    int32_t first_kept;     /* correspondences the first iteration kept                                              */
    int32_t last_kept;      /* ... the last iteration that looked for correspondences kept                           */
    int32_t min_kept;       /* the least any iteration kept                                                          */
    int32_t stopped_few;    /* 1: the ICP stopped with fewer than three (step 1 or step 5)                           */
    float last_median;      /* m of the last iteration that took one (step 2); 0 when none did                       */
    int32_t reserved[3];
} cd_icp_reject_stats;
int cd_set_icp_median_rejection(cd_context* ctx, double factor);
int cd_get_icp_median_rejection(const cd_context* ctx, double* factor);
int cd_icp_reject_struct_size(void);   /* sizeof(cd_icp_reject_stats) (cd_struct_size's list is closed) */
/* Indexed like cd_get_cluster_results (the stats of the template whose result the cluster kept); after a stand-alone cd_icp
 * the result is at frame 0, index 0.  A cluster that was never run (fewer than three points) has zeros.  Returns the number
 * copied; CD_ERR_INVALID_ARG when the call ran with the mode off, has been invalidated by another compute call, or had no such
 * frame. */
int cd_get_cluster_reject_stats(const cd_context* ctx, int frame, int first, int count, cd_icp_reject_stats* out);
/* Host only (no context, no GPU): steps 2 and 3 over the n >= 1 squared distances of K0 (non-negative, +inf allowed; a NaN or a
 * signed value gives CD_ERR_INVALID_ARG, as does a factor the setter would refuse or 0).  median and thr may be NULL. */
int cd_icp_median_threshold(const float* d2, int n, double factor, float* median, double* thr);

/* Reciprocal correspondences inside the ICP: opt-in, off by default.  Canonical rule C22;
 * perception_amd/icp_reciprocal.py is the rule in numpy and the device equals it bit for bit.  It restates
 * pcl::IterativeClosestPoint::setUseReciprocalCorrespondences(true) (CorrespondenceEstimation::determineReciprocalCorrespondences)
 * as commonly described; parity with a real PCL is unpinned (k-d tree ties).  It changes results: the step is estimated from
 * fewer correspondences.  It is the rejection without a number to tune, meant for sources that hold points the template has no
 * counterpart for, from a start near the template: far from it every source point picks the same few template points, only one
 * of each survives, and the ICP stops or crawls (README, "Reciprocal correspondences").
 * With the mode on, every ICP iteration takes its correspondences by rule C5 - source point i of the n current positions X gets
 * template point j_i and the float32 d2_i; rule C8's bound leaves the set K0 (every point when it bounds nothing).  Then
 *   1. |K0| < 3 stops the ICP as rule C8 does (T = identity, converged = 0, Tfinal and iterations as they were);
 *   2. for every i of K0, r_i = the index of the source point nearest to q = tpl[j_i] among ALL n current positions, inside K0 or
 *      not: d2(q, x) = (dx dx + dy dy) + dz dz in float32 with dx = q.x - x.x, every operation rounded on its own; ties to the
 *      lowest source index;
 *   3. i is kept iff r_i == i: no i' has d2(q, X_i') < d2(q, X_i) and no i' < i has an equal one;
 *   4. fewer than three kept: the stop of step 1;
 *   5. the 16 moment sums of rule C4, the MSE of the convergence tests and the solve's n are over the kept ones only.
 * X <- T X moves every point, getFitnessScore() is over all points and unbounded, `accepted`, the pose and the order of the
 * convergence tests are untouched.
 *
 * cd_set_icp_reciprocal: context state, as the correspondence distance is; applies to every ICP of the following cd_icp and fused
 * calls, the coarse level of rule C18 included.  on == 0 turns the mode off (the default: every record, launch and kernel is what
 * it was); any other value turns it on.  With the mode on every live cluster goes to the mode's own driver (the sliced loop with
 * k_icp_recip behind every iteration, at most n^2 pair tests per cluster and iteration); CUBOID_ICP_LATTICE / CUBOID_ICP_MODE do
 * not apply.  Together with plane-weighted ICP (rule C17) or median-distance rejection (rule C19) every ICP entry point returns
 * CD_ERR_INVALID_ARG before anything is launched (PCL runs its rejectors on what the reciprocal estimation left; that composition
 * is not offered).  In cd_icp a stop returns CD_ERR_FEW_CORRESPONDENCES with out filled, as under rule C8; in a batch it is a
 * result, the frame stays CD_OK. */
typedef struct cd_icp_recip_stats {
    int32_t first_kept;     /* correspondences the first iteration kept                                              */
    int32_t last_kept;      /* ... the last iteration that looked for correspondences kept                           */
    int32_t min_kept;       /* the least any iteration kept                                                          */
    int32_t stopped_few;    /* 1: the ICP stopped with fewer than three (step 1 or step 4)                           */
    int32_t last_n0;        /* |K0| of the last iteration that looked for correspondences                            */
    int32_t reserved[3];
} cd_icp_recip_stats;
int cd_set_icp_reciprocal(cd_context* ctx, int on);
int cd_get_icp_reciprocal(const cd_context* ctx, int* on);
int cd_icp_recip_struct_size(void);   /* sizeof(cd_icp_recip_stats) (cd_struct_size's list is closed) */
/* Indexed like cd_get_cluster_results (the stats of the template whose result the cluster kept); after a stand-alone cd_icp
 * the result is at frame 0, index 0.  A cluster that was never run (fewer than three points) has zeros.  Returns the number
 * copied; CD_ERR_INVALID_ARG when the call ran with the mode off, has been invalidated by another compute call, or had no such
 * frame. */
int cd_get_cluster_recip_stats(const cd_context* ctx, int frame, int first, int count, cd_icp_recip_stats* out);
/* Host only (no context, no GPU): one iteration's steps 1 - 3 by brute force for n >= 1 source positions and m >= 1 template
 * points (x, y, z float32, the strides in bytes, multiples of 4 and >= 12).  Rule C5's correspondences are searched here (ties
 * to the lowest template index) and written to nn and d2 when those are not NULL; d2_max: rule C8's threshold on d2
 * (cd_icp_correspondence_threshold; +inf: unbounded; a NaN or a negative value gives CD_ERR_INVALID_ARG).  keep[i] = 1 for a kept
 * point, else 0.  Returns |K0|; with |K0| < 3 nothing is tested and keep marks K0 itself. */
int cd_icp_reciprocal_mask(const void* src_xyz, size_t src_stride, int n, const void* tpl_xyz, size_t tpl_stride, int m, float d2_max,
                           int32_t* nn, float* d2, uint8_t* keep);

/* Table prism: keep only the object points above the convex hull of the plane inliers (pcl::ConvexHull of the inliers followed
 * by pcl::ExtractPolygonalPrismData): opt-in, off by default.  Canonical rule C20; perception_amd/table_prism.py
 * is the rule in numpy and the device equals it bit for bit - the kept set, the record and the hull.  Parity with a real PCL is
 * unpinned (its hull is qhull's, in floating point; here the hull is one of integers and its boundary counts as inside).  For
 * the refined plane (a, b, c, d) as float32, the plane inliers, a cloud and the limits height_min <= height_max:
 *   1. all arithmetic is double, every product and sum rounded on its own in the order written.  s = -1 if d < 0, else +1;
 *      n = s (a, b, c), dd = s d: the sensor at the origin is on the positive side (PCL's default viewpoint);
 *   2. h(p) = ((n0 x + n1 y) + n2 z) + dd;
 *   3. p' = p - h n per component, as x - (h n0);
 *   4. the axis k0 = argmax(|a|, |b|, |c|) (float32 compares, the lowest index on a tie) is dropped; (k1, k2): the others, ascending;
 *   5. u = floor(p'[k1] 65536), v = floor(p'[k2] 65536), clamped to [-2^29, 2^29 - 1] (a NaN to -2^29), int32; integers from here;
 *   6. the hull: the strict vertices of the convex hull of the inliers' (u, v) - no duplicate, no point on an edge between two
 *      others - counter-clockwise from the lexicographically smallest.  Fewer than 3: nothing is kept.  More than
 *      CD_PRISM_MAX_HULL: the record says overflow, reports no vertex, and nothing is kept;
 *   7. a point is kept iff height_min <= h <= height_max and cross(B - A, P - A) >= 0 for every hull edge A -> B (int64); the
 *      kept points stay in their order, whole records;
 *   8. the record below.  n_before = n_kept + n_below + n_above + n_outside.
 * All plane inliers make the hull: a surface at table level beside the table extends it, as in PCL when every inlier is used.
 *
 * cd_set_table_prism: context state, as the outlier filter's.  enable = 0 turns the step off (the default: no kernel of the fused
 * calls changes and every output is byte for byte what it was).  Limits that are not finite or not min <= max give
 * CD_ERR_INVALID_ARG and the setting stays.  With the step on, every fused call runs it on each frame's object cloud between S3
 * and the outlier filter (PCL's tabletop order: the prism, then cleaning), and everything behind it takes the kept cloud:
 * the filter, clustering, the surface and cluster guesses, ICP, n_objects, the `labels` output,
 * cd_get_frame_cloud(CD_CLOUD_OBJECTS) and cd_get_cluster_points.  The label calls (rule C15) give a voxel the prism removed
 * CD_LABEL_GATED.  A frame without a plane passes untouched: n_kept = n_before and every other field 0.
 * CD_PRISM_LDS_POINTS: the pruned inliers the kernel keeps in LDS (more are read from global memory). */
#define CD_PRISM_MAX_HULL 1024
#define CD_PRISM_LDS_POINTS 4096
typedef struct cd_prism_stats {
    int32_t n_before;       /* points of the cloud                                                                   */
    int32_t n_kept;
    int32_t n_below;        /* h < height_min                                                                        */
    int32_t n_above;        /* not below and not h <= height_max (a NaN height counts here)                          */
    int32_t n_outside;      /* passed the height test, outside the hull (or no hull of three vertices)               */
    int32_t hull_vertices;  /* 0 on overflow                                                                         */
    int32_t axis_u, axis_v; /* k1, k2                                                                                */
    int32_t overflow;       /* 1: more than CD_PRISM_MAX_HULL hull vertices                                          */
    int32_t reserved[3];
} cd_prism_stats;
int cd_set_table_prism(cd_context* ctx, int enable, double height_min, double height_max);
int cd_get_table_prism(const cd_context* ctx, int* enable, double* height_min, double* height_max);
int cd_prism_struct_size(void);   /* sizeof(cd_prism_stats) (cd_struct_size's list is closed) */
/* What the step did to `frame` of the last fused call, and that frame's hull (u, v interleaved; *n = its vertices, also when
 * capacity is too small: CD_ERR_CAPACITY then).  CD_ERR_INVALID_ARG when that call ran without the step, has been invalidated
 * (the validity rule of cd_get_cluster_results) or had no such frame. */
int cd_get_prism_stats(const cd_context* ctx, int frame, cd_prism_stats* out);
int cd_get_prism_hull(cd_context* ctx, int frame, int32_t* uv, int capacity, int* n);
/* The step as a call of its own: the kept indices ascending, like cd_outlier_filter.  plane_xyz: the n_plane plane inliers
 * (plane_stride bytes apart), coeff the plane.  stats and hull_uv may be NULL (hull_capacity vertices; fewer than the hull has
 * gives CD_ERR_CAPACITY).  Out-of-range arguments give CD_ERR_INVALID_ARG before anything is launched; n or n_plane above the
 * context's max_points CD_ERR_CAPACITY; capacity < kept CD_ERR_CAPACITY with *out_n = kept.  The context's own setting is neither
 * read nor changed; like every compute call it invalidates the read-backs of the last fused call. */
int cd_table_prism(cd_context* ctx, const void* plane_xyz, size_t plane_stride, int n_plane, const float coeff[4], const void* xyz,
                   size_t stride_bytes, int n, double height_min, double height_max, int32_t* out_indices, int capacity, int* out_n,
                   cd_prism_stats* stats, int32_t* hull_uv, int hull_capacity);
/* Host only (no context, no GPU).  cd_prism_project: steps 1 - 5 of one point - height, uv[2], axes[2] = (k1, k2); any output may
 * be NULL.  cd_prism_hull_host: step 6 without the cap by a monotone chain over n >= 0 points (u, v interleaved): *n_hull = the
 * hull's vertices, the first min(*n_hull, capacity) written; CD_ERR_CAPACITY when they did not all fit. */
int cd_prism_project(const float coeff[4], const float xyz[3], double* height, int32_t uv[2], int32_t axes[2]);
int cd_prism_hull_host(const int32_t* uv, int n, int32_t* hull, int capacity, int* n_hull);

/* Two-way registration score of a (cluster, template) pair: how much of the template the aligned cluster accounts for, beside how
 * well the cluster lies on the template - what PCL users take from getFitnessScore(max_range) and
 * TransformationValidationEuclidean.  Opt-in, off by default.  Canonical rule C21; perception_amd/pair_score.py is
 * the rule in numpy and the device equals it bit for bit.  Parity with a real PCL is unpinned (its validation has thresholds of
 * its own, float sums and a k-d tree).  For the cluster's n points src as extracted (cd_get_cluster_points(aligned = 0)), the
 * result's T, the m points tpl of its template_slot and a range d (a double, finite, > 0):
 *   1. A_i = T src_i, once, in float32, every product and sum rounded on its own: ((T[4r] x + T[4r+1] y) + T[4r+2] z) + T[4r+3] for
 *      row r - the order of cd_get_cluster_points(aligned != 0) when the kept pass is no longer resident, so A is that read-back.
 *      The ICP's iterated cloud is not used: the score is a function of (src, T, tpl, d);
 *   2. d2(p, q) = (dx dx + dy dy) + dz dz in float32; f_i = min_j d2(A_i, tpl_j), r_j = min_i d2(tpl_j, A_i): exact minima over
 *      all pairs, no index, so neither order nor ties matter;
 *   3. tau = rule C8's threshold of d (cd_icp_correspondence_threshold); a distance equal to tau is inside;
 *   4. n_source_in = #{i: f_i <= tau}, n_template_in = #{j: r_j <= tau};
 *   5. three rule-C4 sums of fixq(min(v, 256), 36), 64-bit integers: of f over the inside source points, of r over the inside
 *      template points and of r over all m.  A term is clamped to 256 m^2 (a neighbour 16 m away; inside rule C4's range,
 *      |coordinate| <= 64, a d2 reaches 49152) so that 2^19 terms of at most 2^44 sum to at most 2^63, inside an unsigned 64-bit integer.  forward_fitness_in and
 *      reverse_fitness_in: (double) S 2^-36 / count, 0 for a count of 0; reverse_fitness = (double) S_all 2^-36 / m;
 *   6. coverage = n_template_in / m, inlier_fraction = n_source_in / n, in double;
 *   7. valid = accepted && coverage >= min_coverage && inlier_fraction >= min_inlier_fraction (the boundary is valid);
 *   8. status, the first that applies: CD_ERR_NO_TEMPLATE for an empty slot, CD_ERR_FEW_CORRESPONDENCES for n < 3 (a cluster whose
 *      ICP stopped under rule C8 keeps its T and is scored like any other), CD_ERR_CAPACITY for n or m above 2^19,
 *      CD_ERR_INVALID_ARG for a non-finite entry of T or a non-finite coordinate of tpl or A.  Such a record holds n_source,
 *      n_template, status and zeros.
 * A template's hidden faces count as uncovered (no visibility reasoning), which is why min_coverage is a setting.
 *
 * cd_set_pair_score: context state.  enable = 0 (the default): a fused call launches nothing more and every output is byte for
 * byte what it was.  max_range not finite or <= 0, or a fraction outside [0, 1] (NaN included): CD_ERR_INVALID_ARG and the
 * setting stays.  With the mode on, every fused call scores each cluster result against the slot it reports, after its ICP;
 * cd_frame_result, cd_cluster_result (accepted, fitness, poses, the slot) and every other read-back are unchanged. */
#define CD_PAIR_SCORE_RANGE_DEFAULT 0.005
#define CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT 0.5
#define CD_PAIR_SCORE_MIN_INLIER_DEFAULT 0.8
typedef struct cd_pair_score {
    int32_t n_source;           /* n                                                                                     */
    int32_t n_source_in;        /* source points whose nearest template point is within the range                        */
    int32_t n_template;         /* m                                                                                     */
    int32_t n_template_in;      /* template points whose nearest aligned source point is within the range                */
    int32_t valid;              /* step 7                                                                                */
    int32_t status;             /* step 8                                                                                */
    double forward_fitness_in;  /* mean f over the inside source points                                                  */
    double reverse_fitness_in;  /* mean r over the inside template points                                                */
    double reverse_fitness;     /* mean r over the whole template (terms clamped to 256)                                 */
    double coverage;            /* n_template_in / m                                                                     */
    double inlier_fraction;     /* n_source_in / n                                                                       */
} cd_pair_score;
int cd_set_pair_score(cd_context* ctx, int enable, double max_range, double min_coverage, double min_inlier_fraction);
int cd_get_pair_score(const cd_context* ctx, int* enable, double* max_range, double* min_coverage, double* min_inlier_fraction);
int cd_pair_score_struct_size(void);   /* sizeof(cd_pair_score) (cd_struct_size's list is closed) */
/* The scores of the last fused call's cluster results, indexed like cd_get_cluster_results (clusters beyond
 * CD_MAX_CLUSTERS_PER_FRAME included).  Returns the number copied; CD_ERR_INVALID_ARG when the call ran with the mode off, has
 * been invalidated by another compute call, or had no such frame.  cd_icp alone produces no score. */
int cd_get_cluster_pair_scores(const cd_context* ctx, int frame, int first, int count, cd_pair_score* out);
/* One pair from host points, on the GPU, without a fused call: src_xyz (n points, stride_bytes apart) against the template of
 * `slot` under T (row-major 4x4 float32).  The thresholds are the call's own (the context's setting is neither read nor changed);
 * `accepted` is the flag step 7 starts from.  A bad argument (a null pointer, n < 0, a bad stride or slot, thresholds the setter
 * would refuse): CD_ERR_INVALID_ARG; n above the context's max_points: CD_ERR_CAPACITY.  Otherwise CD_OK with the record's own
 * status in out->status.  Like every compute call it invalidates the read-backs of the last fused call. */
int cd_pair_score_points(cd_context* ctx, int slot, const void* src_xyz, size_t stride_bytes, int n, const float T[16], double max_range,
                         double min_coverage, double min_inlier_fraction, int accepted, cd_pair_score* out);
/* Host only (no context, no GPU): the same rule by two plain loops over all pairs, through the arithmetic header the kernel uses. */
int cd_pair_score_host(const void* tpl_xyz, size_t tpl_stride, int m, const void* src_xyz, size_t src_stride, int n, const float T[16],
                       double max_range, double min_coverage, double min_inlier_fraction, int accepted, cd_pair_score* out);

/* Pose information of a (cluster, lattice template) pair: does the data pin the pose down at all?  A cluster that sees one face of
 * a cuboid lies perfectly on the template wherever it slides within that face and however it turns about the face's normal; a
 * two-face view leaves the translation along the common edge free.  Fitness, rule C14 and rule C21 all ask whether the cluster
 * lies on the template and pass such poses; this rule reports which of the six directions of a small rigid motion the
 * correspondences constrain, by how many points' worth, and the covariance of the pose over the constrained ones.  Opt-in, off by
 * default, lattice templates only (cd_template_lattice_faces > 0).  Canonical rule C23; perception_amd/pose_info.py
 * is the rule in numpy, with every association, and the device equals it bit for bit.  It counts what the template's SURFACES
 * constrain and nothing else: the outline of a partial view adds nothing, and hidden faces are not reasoned about.
 * For the cluster's n points src as extracted, the result's T, the slot's template, a range d and a support min_support (doubles,
 * finite, > 0), everything in the template's frame:
 *   1. A_i = T src_i in float32, rule C21's step 1;
 *   2. rule C5's neighbour q_i of A_i, its squared distance and w_i, the constant axis of q_i's face; i is kept iff d2_i <= rule
 *      C8's threshold of d (the boundary inside); n_in the kept, n_face[a] the kept with w = a;
 *   3. centre c0 = float32 (min + max) * 0.5f per axis of the template's bounding box, length L = half its diagonal (double, from
 *      the float32 extents), both fixed at cd_set_template; p_i = A_i - c0 in float32;
 *   4. per kept point with a = w_i, b and c the next two axes cyclically and r = q_a - A_a, the float32 terms p_c, p_b, p_c p_c,
 *      p_b p_b, p_c p_b and r r, summed per axis as rule-C4 64-bit integers (2^32; r r: 2^36) next to the counts: order-free;
 *   5. in double, the 6 x 6 information matrix H over x = (L omega, t) of the motion A' = A + omega x (A - c0) + t: the row of
 *      point i is ((p_i x e_w) / L, e_w).  Its eigenvalues read as "how many points constrain this direction";
 *   6. H's eigenvalues ascending with their vectors, by a cyclic Jacobi of a fixed pair order and sweep count; a vector's
 *      component of largest magnitude is positive;
 *   7. n_constrained = #{k: eigenvalue k >= min_support}; sigma2 = the mean r r of the kept points; the covariance of (omega, t) =
 *      sigma2 D (sum over the constrained k of v_k v_k^T / lambda_k) D with D = diag(1/L, 1/L, 1/L, 1, 1, 1).  Free directions
 *      are ABSENT from it, not infinite: n_constrained says so.  weakest = v_0, the twist (L omega, t) the data says least about;
 *   8. well_posed = accepted && n_constrained == 6;
 *   9. status, the first that applies: CD_ERR_NO_TEMPLATE for an empty slot, CD_ERR_INVALID_ARG for a slot that is not a lattice or
 *      a non-finite entry of T or coordinate of A, CD_ERR_FEW_CORRESPONDENCES for n_in < 3, CD_ERR_CAPACITY for n above 2^19.  Such
 *      a record holds the counts (n_source; n_in and n_face where the points were looked at), the status and zeros.
 *
 * cd_set_pose_info: context state.  enable = 0 (the default): a fused call launches nothing more and every output is byte for byte
 * what it was.  max_range or min_support not finite or <= 0: CD_ERR_INVALID_ARG and the setting stays.  With the mode on, every fused
 * call examines each cluster result against the slot it reports, after its ICP and after rule C21's step; every other record and
 * read-back is unchanged. */
#define CD_POSE_INFO_RANGE_DEFAULT 0.005
#define CD_POSE_INFO_MIN_SUPPORT_DEFAULT 8.0
typedef struct cd_pose_info {
    int32_t n_source;          /* n                                                                                      */
    int32_t n_in;              /* kept correspondences                                                                   */
    int32_t n_face[3];         /* ... whose face has the constant axis x / y / z                                         */
    int32_t n_constrained;     /* eigenvalues >= min_support                                                             */
    int32_t well_posed;        /* step 8                                                                                 */
    int32_t status;            /* step 9                                                                                 */
    double eigenvalues[6];     /* ascending, in points                                                                   */
    double eigenvectors[36];   /* row k = v_k over (L omega, t)                                                          */
    double weakest[6];         /* v_0                                                                                    */
    double sigma2;             /* mean squared normal residual of the kept points                                        */
    double covariance[36];     /* row-major over (omega, t), template frame, rotation about `centre`                     */
    double centre[3];          /* c0                                                                                     */
    double length;             /* L                                                                                      */
} cd_pose_info;
int cd_set_pose_info(cd_context* ctx, int enable, double max_range, double min_support);
int cd_get_pose_info(const cd_context* ctx, int* enable, double* max_range, double* min_support);
int cd_pose_info_struct_size(void);   /* sizeof(cd_pose_info) (cd_struct_size's list is closed) */
/* The records of the last fused call's cluster results, indexed and invalidated exactly like cd_get_cluster_pair_scores. */
int cd_get_cluster_pose_info(const cd_context* ctx, int frame, int first, int count, cd_pose_info* out);
/* One pair from host points, on the GPU, without a fused call; the arguments are checked like cd_pair_score_points' (a setting the
 * setter would refuse: CD_ERR_INVALID_ARG; n above the context's max_points: CD_ERR_CAPACITY).  CD_OK with the record's own
 * status in out->status. */
int cd_pose_info_points(cd_context* ctx, int slot, const void* src_xyz, size_t stride_bytes, int n, const float T[16], double max_range,
                        double min_support, int accepted, cd_pose_info* out);
/* Host only (no context, no GPU): rule C5's neighbour by brute force, the faces from cd_lattice_detect, the arithmetic header the
 * kernel uses. */
int cd_pose_info_host(const void* tpl_xyz, size_t tpl_stride, int m, const void* src_xyz, size_t src_stride, int n, const float T[16],
                      double max_range, double min_support, int accepted, cd_pose_info* out);
/* Host only, in double: the covariance of the published pose P = T^-1 (the template in the camera frame) in the order of
 * geometry_msgs/PoseWithCovariance - position, then rotation about the fixed axes of the parent frame - as J S J^T with S =
 * info->covariance, R_P the rotation of P and J = [[-R_P [c0]x, -R_P], [-R_P, 0]] over (omega, t).  Free directions are absent
 * from S and so from the result: n_constrained says so.  NULL pointer: CD_ERR_INVALID_ARG. */
int cd_pose_info_ros_covariance(const cd_pose_info* info, const float T[16], double out36[36]);

/* Box fit: a resting cuboid's dimensions, yaw and centre from the table plane and the points of its cluster - no template, no
 * search, no iteration.  Every registration path needs a template of the right size uploaded beforehand; this step measures the
 * object instead: its height above the table, the minimum-area rectangle of its top face's footprint, hence L, W, H, the long
 * axis and the centre.  Opt-in, off by default.  Canonical rule C24; perception_amd/box_fit.py is the rule in
 * numpy, with every association, and the device and cd_box_fit_host equal it bit for bit.  The rule assumes that the cuboid rests
 * on the plane with a face up: a tilted or stacked box gets a record whose rectangularity says so, and nothing else.
 * For the plane (a, b, c, d) as float32, n float32 points and band (a double, finite, 0 < band <= 64), all real arithmetic in
 * double, every product and sum rounded on its own in the order written:
 *   1. (nrm, dd) is rule C20's step 1; h(p) = ((nrm0 x + nrm1 y) + nrm2 z) + dd;
 *   2. k0 is rule C20's step 4, k1 = (k0 + 1) mod 3; t_j = [j == k1] - (nrm[k1] nrm_j); len = sqrt((t0 t0 + t1 t1) + t2 t2);
 *      eu_j = t_j / len; ev = nrm x eu, each component as (nrm_a eu_b) - (nrm_b eu_a): a metric basis of the plane;
 *   3. per point qh = floor(h 65536), u = floor(((eu0 x + eu1 y) + eu2 z) 65536), v likewise with ev, clamped and NaN-mapped as rule
 *      C20's step 5, int32; everything from here on is integer unless a conversion is written;
 *   4. k = 1 + n / 64, href = the k-th largest qh; top = {qh >= href - floor(band 65536)};
 *      height = ((double) sum_top qh / (double) n_top) / 65536;
 *   5. the hull of the top set's (u, v): rule C20's step 6, capped at CD_PRISM_MAX_HULL vertices;
 *   6. per hull edge i (A = H[i], e = H[i + 1 mod m] - A) over all hull vertices P: along = (P - A) . e, across = e_u (P - A)_v -
 *      e_v (P - A)_u; w, g = max - min of each, l2 = e . e; area_i = ((double) w (double) g) / (double) l2; the smallest wins, a
 *      tie goes to the lowest i;
 *   7. s = sqrt((double) l2), p = ((double) w / s) / 65536, q = ((double) g / s) / 65536; dims = (max(p, q), min(p, q), height);
 *      the long axis in (u, v) is e when p >= q, else (-e_v, e_u), negated when its u component is negative (or zero with a negative
 *      v component), divided by s;
 *   8. the rectangle's centre (cu, cv) = A + ((amin + amax) / (2 l2)) e + ((cmin + cmax) / (2 l2)) (-e_v, e_u);
 *      centre = (cu / 65536) eu + (cv / 65536) ev + (height / 2 - dd) nrm; pose: row-major 4 x 4, box -> camera, columns ex (the
 *      long axis lifted through eu, ev), ey = nrm x ex, nrm, centre - cd_cluster_result.pose's convention; rounded to float32 it
 *      is an Rt that cd_surface_guess takes;
 *   9. area = area_min / 65536^2; rectangularity = hull area (integer shoelace sum, halved in double, / 65536^2) / area;
 *      height_ref = href / 65536;
 *  10. status, a result and not a failure of the call: n < 3: CD_ERR_FEW_CORRESPONDENCES; a non-finite coordinate or |coordinate|
 *      > 64: CD_ERR_INVALID_ARG; no plane (a frame without one, a non-finite coefficient, a = b = c = 0) or a hull of fewer than 3
 *      vertices: CD_ERR_NO_MODEL; more than CD_PRISM_MAX_HULL vertices: CD_ERR_CAPACITY with overflow = 1 and hull_vertices = 0.
 *      Such a record holds the counts reached so far and zeros elsewhere.
 * CD_BOX_FIT_LDS_POINTS: the points of a cluster whose (qh, u, v) the kernel keeps in LDS; a larger cluster is quantised again from
 * global memory in every pass (the same integers). */
#define CD_BOX_FIT_BAND_DEFAULT 0.006
#define CD_BOX_FIT_LDS_POINTS 2048
typedef struct cd_box_fit {
    int32_t n;                 /* points of the cluster                                                                  */
    int32_t n_top;             /* ... in the top set                                                                     */
    int32_t hull_vertices;     /* strict vertices of the top set's hull                                                  */
    int32_t edge;              /* the hull edge the rectangle lies along                                                 */
    int32_t status;            /* step 10                                                                                */
    int32_t overflow;          /* the hull has more than CD_PRISM_MAX_HULL vertices                                      */
    int32_t match_slot;        /* the selection on (cd_set_box_select): cd_box_fit_match's slot of a CD_OK record; else -1 */
    int32_t reserved;
    double height_ref;         /* href / 65536                                                                           */
    double dims[3];            /* L >= W, H, metres                                                                      */
    double pose[16];           /* step 8                                                                                 */
    double area;               /* of the rectangle, square metres                                                        */
    double rectangularity;     /* hull area / rectangle area, 1 for a rectangle                                          */
    double match_cost;         /* ... and its cost; 0 with the selection off                                             */
} cd_box_fit;
int cd_box_fit_struct_size(void);   /* sizeof(cd_box_fit) (cd_struct_size's list is closed) */
/* Host only (no context, no GPU): the rule through the arithmetic header the kernel uses.  CD_OK with the record's own status in
 * out->status; a NULL pointer (coeff, out, xyz with n > 0), n < 0, a stride below 12 or a band the rule refuses:
 * CD_ERR_INVALID_ARG, nothing written. */
int cd_box_fit_host(const float coeff[4], const void* xyz, size_t stride_bytes, int n, double band, cd_box_fit* out);
/* n_sets point sets on the GPU in one launch, without a fused call: set i is the points offsets[i] .. offsets[i + 1] of xyz
 * (ascending, as cd_shape_frames) against the plane coeff[4 i .. 4 i + 3].  out[i] is its record.  A NULL coeff / offsets / out (or
 * xyz with points to read), n_sets <= 0, a stride below 12 or not a multiple of 4, offsets that are negative or descend, a band
 * the rule refuses: CD_ERR_INVALID_ARG. */
int cd_box_fit_points(cd_context* ctx, const float* coeff, const void* xyz, size_t stride_bytes, const int32_t* offsets, int n_sets, double band,
                      cd_box_fit* out);
/* cd_set_box_fit: context state.  enable = 0 (the default): a fused call launches nothing more and every output is byte for byte
 * what it was; the band is then not looked at and stays, and the selection below goes off with the step.  enable != 0 with a band
 * the rule refuses: CD_ERR_INVALID_ARG and the setting stays.  With the step on, every fused call fits each cluster as clustered,
 * right after the cluster hand-over (after the table prism and the outlier filter when those are on), against its frame's plane;
 * every other record and read-back is unchanged.  cd_get_cluster_box_fits: the records of the last fused call's clusters, indexed and
 * invalidated exactly like cd_get_cluster_pair_scores. */
int cd_set_box_fit(cd_context* ctx, int enable, double band);
int cd_get_box_fit(const cd_context* ctx, int* enable, double* band);
int cd_get_cluster_box_fits(const cd_context* ctx, int frame, int first, int count, cd_box_fit* out);
/* cd_set_box_select: context state, off by default.  slot_dims[s] = (length, width, height) of the template in slot s; needs the box
 * fit on (else CD_ERR_INVALID_ARG, as for a NULL slot_dims, a non-finite entry, a tolerance that is not finite or negative; the
 * setting stays).  enable = 0 needs no other argument.  It acts only in a fused call with template_slot == -1 and more than one
 * loaded slot: a cluster whose record is CD_OK and matches a loaded slot (cd_box_fit_match over the loaded slots, this tolerance)
 * is registered against that slot alone, and its result is, bit for bit, what the same call with template_slot = that slot gives
 * the cluster; every other cluster runs against every loaded slot, as without the selection.  It costs one device -> host read of
 * the box records ahead of the ICP.  A call in which no cluster matches is the call without the selection, launch for launch.
 * With the selection on every CD_OK record of a fused call carries match_slot / match_cost. */
int cd_set_box_select(cd_context* ctx, int enable, const double slot_dims[CD_MAX_TEMPLATES][3], double tolerance);
int cd_get_box_select(const cd_context* ctx, int* enable, double slot_dims[CD_MAX_TEMPLATES][3], double* tolerance);
/* Host only: which of the slots has the fitted dimensions?  slot_dims[s] = (length, width, height) of slot s, considered when
 * bit s of loaded_mask is set; a slot's first two are sorted descending; cost = max(|L - Ls|, |W - Ws|, |H - Hs|) in double.  The
 * lowest cost wins, a tie goes to the lowest slot; *slot = -1 when no slot is considered (*cost = 0) or the best cost exceeds
 * tolerance (*cost is that cost).  NULL dims / slot_dims / slot / cost or a tolerance that is NaN or negative:
 * CD_ERR_INVALID_ARG. */
int cd_box_fit_match(const double dims[3], const double slot_dims[CD_MAX_TEMPLATES][3], uint32_t loaded_mask, double tolerance, int32_t* slot,
                     double* cost);

/* S7 helpers: tf::Matrix3x3::getRotation + position (icp.cpp:55-82) and the 8 bbox
 * corners in the order of icp.cpp:99-106 transformed by pose.cast<float>() (icp.cpp:110). */
void cd_pose_to_position_quaternion(const double pose[16], double position[3],
                                    double quat_xyzw[4]);
void cd_bbox_corners(const double pose[16], double length, double width, double height,
                     float corners_xyz[24]);

/* Timing of the last cd_process_batch* call, milliseconds per stage measured with HIP
 * events on the context's stream: [0] crop+voxel (and, for depth input, the deprojection and - CD_BBOX_COLOR - the colour
 * gate's stage), [1] plane, [2] extract+cluster, [3] icp, [4] total device time.  Also the ICP kernel's launch count and summed time. */
typedef struct cd_timing {
    float stage_ms[5];
    float icp_kernel_ms;
    int32_t icp_kernel_launches;
    int32_t icp_pair_tests_lo, icp_pair_tests_hi; /* 64-bit count of point-pair distance tests */
    int32_t icp_persist_gave_up;                  /* single-launch ICPs of this call that gave up at a grid barrier and were redone by the
                                                   * multi-launch loop (same results, tens of ms slower): 0 in a healthy run           */
    int64_t algorithmic_bytes;                    /* B_alg of SURVEY 8(d) for this batch */
    int64_t icp_algorithmic_bytes;                /* the S6 term of B_alg: sum 12*M + 12*N_s*(I_c+1) */
    int32_t scan_retries;                         /* 1 when this call was redone because a chained scan reported a stall (cannot happen on
                                                   * its own since the scans take their tile ids from atomic tickets; the redo runs with
                                                   * the device to itself): 0 in a healthy run                                          */
    int32_t icp_regime;                           /* launch shape of the whole-cluster ICP kernel of this call: (clusters in flight per
                                                   * workgroup << 16) | workgroups; 0 = no such launch (sliced driver).  The shape is
                                                   * chosen from the calls in flight on the device (scheduling only: results do not
                                                   * depend on it), so a measurement can say which shape it measured                    */
    int32_t icp_handovers;                        /* running clusters that changed workgroup inside that launch (a call that has the GPU to
                                                   * itself lets workgroups without work take over clusters from those that still have
                                                   * several: scheduling only, results do not depend on it)                             */
    int32_t icp_search;                           /* which nearest-neighbour search the ICPs of this call ran: 0 the pruned searches over an
                                                   * arbitrary template, 1 the closed form for a template that is a union of axis-aligned
                                                   * lattices (every make_cuboid.py template; cd_template_lattice_faces), 2 both (mixed batch).
                                                   * Results do not depend on it                                                            */
    int32_t icp_handover_lost;                    /* a cluster in hand-over between two workgroups was claimed and never arrived, or a waiting
                                                   * workgroup ran out of polls: the call has FAILED with CD_ERR_DEVICE (its records are not
                                                   * complete).  Cannot happen in a healthy launch; 0 otherwise                              */
    float icp_wave_ms;                            /* lattice ICP launches: sum over the launch's workgroups of (lifetime x waves), in
                                                   * wave-milliseconds - what the batch's ICP held of the chip's wave slots (256 CUs x 16
                                                   * waves at this kernel's register count); with batches in flight this, not the launch's
                                                   * duration, is what a batch's ICP costs.  0 for the other ICP drivers                     */
} cd_timing;
int cd_get_timing(const cd_context* ctx, cd_timing* out);

#ifdef __cplusplus
}
#endif
#endif /* CUBOID_HIP_H */
