// context.hpp - what the host units of the library share: the context, the error and launch macros, the per-device locks and
// gates, the small-transfer batch and the declarations of every function that more than one unit calls.  Internal: only the
// units that make up the library driver include it (DESIGN.md lists them).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "device_buffer.hpp"
#include "kernels.hpp"
#include "outlier_math.hpp"
#include "prism_math.hpp"
#include "pair_score_math.hpp"
#include "pose_info_math.hpp"
#include "box_fit_math.hpp"
#include "icp_plane_math.hpp"
#include "icp_reject_math.hpp"
#include "icp_recip_math.hpp"
#include "icp_coarse_plan.hpp"
#include "kept_records.hpp"
#include "shape_frame_math.hpp"
#include "template_prep.hpp"
#include "tunables.hpp"

using namespace cd;


// Rule C15: the sorted keys of the voxel stage are still in d_key[cur] when a fused call returns (nothing after the centroid kernel
// writes d_key / d_val).  Frame f's keys are its first n_runs (by_runs) or n_c entries; `packed`: the bit fields of k_crop_runs
// with their KeyPack, otherwise PCL's idx.  `path` names the crop / voxel path for messages.
struct VoxelKeys {
    int cur = 0, by_runs = 0, packed = 0;
    KeyPack kp = {0, 0, 0, 0, 0, 0};
    const char* path = "none";
};
// What a label call needs of the last fused call besides the device buffers (valid while last_first is not empty)
struct LastCall {
    size_t stride = 0;
    int N = 0, F = 0;
    cd_params prm = {};
    FrameRects rects{nullptr, 0};   // the per-frame rectangles its gate read (device memory that stays until the next fused call)
    bool depth_is_c7 = true;        // false: a mapped call that dropped its untextured points (rule C12's xyz is not rule C7's)
    VoxelKeys keys;
    bool filtered = false;          // rule C16: the call filtered its object clouds (d_omap / d_orec describe them, rows of omap_pitch)
    int omap_pitch = 0;
    bool prism = false;             // rule C20: the call ran the table prism (d_pmap / d_plrec are then the map the label calls take: rows of
                                    // omap_pitch, S3 index -> kept cloud, the filter's map already applied when it ran too)
};

// The streams and events of a context.  A base of cd_context, so that they outlive its buffers: the members of cd_context
// are destroyed (the buffers freed) before this destructor runs.  stream2 / stream3: the streams of the persistent ICP
// launches: the second launch of a mixed-template batch runs beside the first (stream2); with icp_lowprio both are low-priority
// streams, so that CUs that come free go to the short front-end kernels of the other batches in flight before the next
// persistent workgroup
struct cd_streams {
    hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr;
    hipEvent_t ev[8] = {nullptr}, ev2[3] = {nullptr, nullptr, nullptr};
    ~cd_streams() {
        for (auto& e : ev2) if (e) hipEventDestroy(e);
        for (auto& e : ev) if (e) hipEventDestroy(e);
        for (hipStream_t s : {stream2, stream3, stream}) if (s) hipStreamDestroy(s);
    }
};

// Every buffer is an owning member (device_buffer.hpp): allocated in cd_create or grown on first use (GROW), freed with the context.
struct cd_context : cd_streams {
    int device = 0;
    int N = 0, F = 0, T = 0;   // capacities: points per frame, frames, tiles per frame
    char err[512] = {0};
    Tunables tun;
    // input staging (host-pointer API)
    DevBuf<char> d_in;   // (capacity in bytes)
    // depth-image input (cd_process_depth_batch): upload buffers of their own, allocated at the context's capacity on first use
    // (d_in is the deprojection's destination, is re-allocated by ensure_input and is the read-back staging area)
    DevBuf<uint16_t> d_depth;
    DevBuf<uint8_t> d_color;
    // per-frame scalars
    DevBuf<FrameState> d_fs;
    PinBuf<FrameState> h_fs;
    // ordered-compaction tile counters
    DevBuf<int> d_tileA, d_tileB, d_tileK, d_tileC;   // (tileC: the centroid kernel's scan state - its own array, so that one launch can zero every array of a batch up front)
    bool batch_zeroed = false;      // a fused batch call has zeroed the scratch arrays of all its stages in one launch (zero_batch_scratch): the stages skip their own fills
    // point buffers (float4 = x,y,z,rgb bits)
    DevBuf<float4> d_cpt, d_vox, d_obj, d_src0, d_src;
    DevBuf<uint32_t> d_key[2], d_val[2], d_ghist;
    DevBuf<int> d_sstate;   // chained-scan state of the radix passes, [pass][F][scatter tiles][256]
    DevBuf<unsigned long long> d_tile64;   // chained-scan state of k_crop_runs: (points, runs) per tile, [F][T]
    DevBuf<int> d_ticket;   // ticket counters, one per frame (TICKET_PITCH ints apart), of the kernels that scan over tiles (take_ticket, common.hpp): zero between launches
    // RANSAC
    DevBuf<int> d_rnd, d_valid, d_counts, d_active, d_have;
    PinBuf<int> h_valid, h_counts, h_active, h_have;
    std::vector<char> plane_gave_up;   // per frame of the last stage_plane: the sampler's device limits ended it before PCL's loop did (CD_ERR_CAPACITY)
    DevBuf<float4> d_models, d_model;
    PinBuf<float4> h_model, h_models;
    DevBuf<unsigned long long> d_sums;
    PinBuf<unsigned long long> h_sums;
    // extract / cluster
    DevBuf<int> d_plane_idx, d_head, d_next, d_parent, d_csize, d_rank, d_cand, d_sizes, d_label;
    // templates
    DevBuf<float4> d_tpl, d_tlo, d_thi;   // points + per-64-run boxes
    DevBuf<float4> d_tplk, d_tlok, d_thik;   // templates in k-d patch order (sliced path)
    DevBuf<IcpGrid> d_grid;                                       // per template slot
    DevBuf<unsigned short> d_kdmap;                               // k-d patch order -> cell-sorted position (resident templates)
    DevBuf<unsigned short> d_tcell;                               // cell start tables, ICP_CELL_STRIDE entries per slot
    DevBuf<int> d_nn;                                             // last NN index of every ICP source point
    DevBuf<float> d_d2;                                           // its squared distance
    DevBuf<int> d_queue;                                          // ICP work queue heads (one per template group)
    DevBuf<int> d_don;                                            // k_icp_pipe: hand-over control block + mailbox (common.hpp DON_*)
    DevBuf<int> d_wgtab;                                          // k_icp_pipe: {first item, end item, queue} per workgroup
    PinBuf<int> h_wgtab;                                          // its pinned staging copy (3 * 1024 ints)
    PinBuf<int> h_ctl;                                            // pinned: control words of k_icp_persist going up [0..7], coming back [8]
    std::vector<IcpState> st_init;                                // initial ICP states of a persistent launch (kept in case it gives up)
    int scan_retries = 0;                                         // calls of this context that were redone because a chained scan stalled
    int persist_gave_up = 0;                                      // persistent launches of this context that handed over to the multi-launch loop
    int n_cu = 256;
    bool fs_initialised = false;                                  // the device FrameStates hold their initial value (set by the zero launch of a fused batch call)
    DevBuf<int> d_order; PinBuf<int> h_order;                     // clusters, largest first
    int tpl_cap = 0, tpl_used = 0;
    std::shared_ptr<const cd::PreparedTemplate> tpl_prep[CD_MAX_TEMPLATES];   // host copies (shared across contexts)
    int tpl_off[CD_MAX_TEMPLATES] = {0}, tpl_m[CD_MAX_TEMPLATES] = {0};
    bool tpl_gridded[CD_MAX_TEMPLATES] = {false};                // slot has a cell start table
    bool tpl_big[CD_MAX_TEMPLATES] = {false};                    // slot does not fit LDS but has what k_icp_pipe_big needs (cell table, k-d map, superpatches)
    DevBuf<IcpSuper> d_super;                                     // per template slot
    DevBuf<IcpLattice> d_lat;                                     // per template slot: axis tables and faces of a lattice template (nface = 0: none)
    int tpl_faces[CD_MAX_TEMPLATES] = {0};                        // faces of the slot's lattice (0: the generic searches take it)
    // ICP
    DevBuf<IcpCluster> d_cl; PinBuf<IcpCluster> h_cl;
    DevBuf<IcpWork> d_work, d_work2; PinBuf<IcpWork> h_work, h_work2;
    int work_cap = 0;                                             // items the work lists hold
    int cl_cap = 0;                                               // ICP problems the cluster arrays hold (grown on demand)
    DevBuf<int> d_koffx;                                          // offsets of the clusters ranked >= KICP, [round][F][KICP]
    std::vector<cd_cluster_result> last_clusters;                 // every cluster result of the last batch, frame-major
    std::vector<int> last_first;                                  // index of frame f's first cluster in it (F + 1 entries)
    // clouds of the last batch that stay resident for cd_get_frame_cloud / cd_get_cluster_points
    std::vector<int> last_nv, last_no;                            // voxels / object points per frame
    std::vector<long long> last_orig_off, last_al_off;            // per cluster: offset of its points in d_src0; of its aligned points in d_src (-1: not resident)
    bool last_clouds = false;
    // initial guesses (cd_set_frame_guesses), and their device copy (also used for the single guess of cd_params)
    std::vector<float> frame_guess;
    DevBuf<float> d_guess;
    // ICP maximum correspondence distance (cd_set_icp_max_correspondence_distance, rule C8): the distance as set, its float
    // threshold on d2 and whether it bounds anything; d_ncorr: kept-correspondence counts of the sliced / persistent drivers
    double icp_max_dist = std::numeric_limits<double>::infinity();
    float icp_d2_max = std::numeric_limits<float>::infinity();
    int icp_bounded = 0;
    DevBuf<uint32_t> d_ncorr;
    // batched surface-normal estimation (cd_surface_batch, CD_GUESS_SURFACE, stage_surface): FrameStates, plane models and point
    // buffers of its own, allocated on first use, so that the S2 plane, the clouds and the plane indices of a fused call stay
    // as they are; s_pts[0..1]: the current and the next cloud of every frame, rows of s_pitch points
    DevBuf<FrameState> d_sfs; PinBuf<FrameState> h_sfs;
    DevBuf<float4> d_smodel, d_spts[2]; PinBuf<float4> h_smodel;
    DevBuf<int> d_shave, d_sactive, d_sidx; PinBuf<int> h_shave, h_sactive;
    DevBuf<float4> d_ssum; PinBuf<float4> h_ssum;                // [F][3] midpoint sums of the three fits (x, y, z, count bits)
    double surface_thr = 0.015;                                   // cd_set_surface_distance_threshold (surface_normal_estimation.launch)
    std::vector<float> surface_guess;                             // rule C9 guesses of the last CD_GUESS_SURFACE call, 16 per frame
    std::vector<cd_surface_frame_result> last_surface;            // cd_get_surface_results
    std::vector<int32_t> last_surface_status;
    bool last_surface_ok = false;
    // colour gate (rule C10, k_color.hip): the sdiv / hdiv tables, one record and one status per frame (device + pinned mirror),
    // the union-find labels and (images whose packed mask does not fit LDS only) the mask buffers, both allocated on first use
    DevBuf<int> d_ctab, d_cstatus, d_clabel; PinBuf<int> h_cstatus;
    DevBuf<ColorRecord> d_crec; PinBuf<ColorRecord> h_crec;
    DevBuf<uint32_t> d_cmask;
    // where the fused calls' gate takes its rectangle from (cd_set_bbox_source), the rectangles cd_set_frame_bboxes stored and
    // their device copy; call_rects: what the gate kernels of the fused call in flight read (nullptr outside one, and for CD_BBOX_PARAMS)
    int bbox_source = CD_BBOX_PARAMS;
    cd_color_gate_params color_prm;
    std::vector<int32_t> frame_rects;
    DevBuf<int32_t> d_rects; PinBuf<int32_t> h_rects;
    FrameRects call_rects{nullptr, 0};
    std::vector<cd_color_bbox> last_bboxes;                       // cd_get_frame_bboxes
    bool last_bboxes_ok = false;
    // overlay (rule C11, k_overlay.hip): poses, box counts and box records of a draw call, grown on demand (boxes: device + pinned mirror)
    DevBuf<double> d_oposes;
    DevBuf<int32_t> d_onbox;
    DevBuf<OverlayBox> d_obox; PinBuf<OverlayBox> h_obox;
    // pose verification (rule C14, k_verify.hip), all grown on demand: the depth images of the host forms (a buffer nothing else
    // reads or stages through), and per (frame, slot) the pose + dims going up and the record coming back (device + pinned mirror)
    DevBuf<uint16_t> d_vdepth;
    DevBuf<VerifyJob> d_vjob; PinBuf<VerifyJob> h_vjob;
    DevBuf<int32_t> d_vnbox; PinBuf<int32_t> h_vnbox;
    DevBuf<VerifyRecord> d_vrec; PinBuf<VerifyRecord> h_vrec;
    // per-cluster principal frames (rule C13, k_shape.hip), all allocated on first use: the template records of every slot (pinned
    // table, uploaded when a template has changed since), one record per ICP problem of a CD_GUESS_CLUSTER stage (device + pinned
    // mirror), and the points / set list of cd_shape_frames
    DevBuf<ShapeFrame> d_tframe; PinBuf<ShapeFrame> h_tframe;
    ShapeFrame tpl_frame[CD_MAX_TEMPLATES] = {};                  // the slots' records (cd_set_template computes them on the host)
    bool tframe_dirty = true;
    DevBuf<ShapeFrame> d_shape; PinBuf<ShapeFrame> h_shape;
    DevBuf<float4> d_shpts;
    DevBuf<IcpCluster> d_shcl;
    KeptRecords<cd_shape_frame> last_shapes;                      // cd_get_cluster_shape_frames: one per cluster of the last fused call (kept_records.hpp)
    DevBuf<IcpState> d_st; PinBuf<IcpState> h_st;
    DevBuf<unsigned long long> d_acc, d_accf; PinBuf<unsigned long long> h_accf;
    // point labels (rule C15, k_labels.hip): where the voxel stage left its sorted keys (host fields, set at the end of
    // stage_crop_voxel), what the last fused call ran with (set when it publishes its read-backs), and the buffers of the label
    // calls, all grown on demand: the voxel keys and classes of every frame (rows of one pitch), the labels and the label images
    // of the host forms
    VoxelKeys voxel_keys;
    LastCall last_call;
    DevBuf<uint32_t> d_vkey;
    DevBuf<uint8_t> d_vclass, d_plabel, d_tlabel;
    // statistical outlier removal (rule C16, k_outlier.hip): the setting (cd_set_outlier_filter; mean_k = 0: off), and - grown on
    // demand - the map of the last filtered call (one int per point of the unfiltered object cloud, rows of one pitch) and one
    // record per frame (device + pinned mirror); last_outlier: the records behind cd_get_outlier_stats
    int outlier_k = 0, outlier_neg = 0;
    double outlier_mul = 1.0;
    DevBuf<int> d_omap;
    DevBuf<OutlierRecord> d_orec; PinBuf<OutlierRecord> h_orec;
    std::vector<OutlierRecord> last_outlier;
    bool last_outlier_ok = false;
    // plane-weighted ICP (rule C17, k_icp_plane.hip): the setting (cd_set_icp_plane_weight; plane_weight = 0: off), one record per
    // ICP problem of a stage (device + pinned mirror, grown on demand), and what cd_get_cluster_plane_stats reads: one record per
    // cluster of the last fused call, frame-major behind the call's own index (kept_records.hpp; a stand-alone cd_icp: one frame, one record)
    double plane_weight = 0.0, plane_switch = CD_ICP_PLANE_SWITCH_DEFAULT;
    DevBuf<PlaneStats> d_pstat; PinBuf<PlaneStats> h_pstat;
    KeptRecords<cd_icp_plane_stats> last_plane;
    // coarse-to-fine ICP (rule C18, k_icp_coarse.hip): the setting (cd_set_icp_coarse; coarse_stride = 0: off); per stage, grown on
    // demand, the gather table, the final states and fitness sums of the coarse problems and the fine problems' hand-over table
    // (pinned + device), and one stats record per fine problem (device + pinned mirror); and what cd_get_cluster_coarse_stats
    // reads, as last_plane
    int coarse_stride = 0, coarse_min = 0;
    DevBuf<CoarseGather> d_cgather; PinBuf<CoarseGather> h_cgather;
    DevBuf<IcpState> d_cst; PinBuf<IcpState> h_cst;
    DevBuf<unsigned long long> d_caccf; PinBuf<unsigned long long> h_caccf;
    DevBuf<CoarseHand> d_chand; PinBuf<CoarseHand> h_chand;
    DevBuf<CoarseStats> d_cstat; PinBuf<CoarseStats> h_cstat;
    KeptRecords<cd_icp_coarse_stats> last_coarse;
    // median-distance correspondence rejection (rule C19, k_icp_reject.hip): the setting (cd_set_icp_median_rejection; 0: off), one
    // record per ICP problem of a stage (device + pinned mirror, grown on demand), and what cd_get_cluster_reject_stats reads, as
    // last_plane
    double reject_factor = 0.0;
    DevBuf<RejectStats> d_rstat; PinBuf<RejectStats> h_rstat;
    KeptRecords<cd_icp_reject_stats> last_reject;
    // reciprocal correspondences (rule C22, k_icp_recip.hip): the setting (cd_set_icp_reciprocal; 0: off), the keep flag of every
    // ICP source point of a stage (indexed as d_src), one record per ICP problem (device + pinned mirror) - all grown on demand -
    // and what cd_get_cluster_recip_stats reads, as last_plane
    int recip_on = 0;
    DevBuf<uint8_t> d_rkeep;
    DevBuf<RecipStats> d_qstat; PinBuf<RecipStats> h_qstat;
    KeptRecords<cd_icp_recip_stats> last_recip;
    // table prism (rule C20, k_prism.hip): the setting (cd_set_table_prism; prism_on = 0: off), and - grown on demand - the map of
    // the last call with the step (one int per point of the cloud S3 left, rows of one pitch), one record per frame (device +
    // pinned mirror), the same counts in the form the label calls read (d_plrec) and every frame's hull (CD_PRISM_MAX_HULL
    // vertices each, read by cd_get_prism_hull); last_prism: the records behind cd_get_prism_stats
    int prism_on = 0;
    double prism_hmin = 0.0, prism_hmax = 0.5;
    DevBuf<int> d_pmap;
    DevBuf<PrismRecord> d_prec; PinBuf<PrismRecord> h_prec;
    DevBuf<OutlierRecord> d_plrec;
    DevBuf<int32_t> d_phull;
    std::vector<PrismRecord> last_prism;
    bool last_prism_ok = false;
    // two-way registration score (rule C21, k_pair_score.hip): the setting (cd_set_pair_score; pair_on = 0: off), and - grown on
    // demand - the jobs and items of a launch (pinned + device), the pairs' integer rows with the queue word behind them (device +
    // pinned mirror); last_pair: what cd_get_cluster_pair_scores reads, one record per cluster of the last fused call
    int pair_on = 0;
    double pair_range = CD_PAIR_SCORE_RANGE_DEFAULT, pair_min_cov = CD_PAIR_SCORE_MIN_COVERAGE_DEFAULT, pair_min_inl = CD_PAIR_SCORE_MIN_INLIER_DEFAULT;
    DevBuf<PairJob> d_psjob; PinBuf<PairJob> h_psjob;
    DevBuf<PairItem> d_psitem; PinBuf<PairItem> h_psitem;
    DevBuf<unsigned long long> d_psacc; PinBuf<unsigned long long> h_psacc;
    KeptRecords<cd_pair_score> last_pair;
    // pose information (rule C23, k_pose_info.hip): the setting (cd_set_pose_info; pose_on = 0: off), every slot's centre and length
    // (fixed by cd_set_template), and - grown on demand - the items of a launch (pinned + device), the records with the queue word
    // in a buffer of its own (device + pinned mirror); last_pose: what cd_get_cluster_pose_info reads, one record per cluster of the
    // last fused call
    int pose_on = 0;
    double pose_range = CD_POSE_INFO_RANGE_DEFAULT, pose_support = CD_POSE_INFO_MIN_SUPPORT_DEFAULT;
    float tpl_centre[CD_MAX_TEMPLATES][3] = {};
    double tpl_length[CD_MAX_TEMPLATES] = {};
    DevBuf<PoseItem> d_piitem; PinBuf<PoseItem> h_piitem;
    DevBuf<cd_pose_info> d_pirec; PinBuf<cd_pose_info> h_pirec;
    DevBuf<int> d_piqueue;
    KeptRecords<cd_pose_info> last_pose;
    // box fit (rule C24, k_box_fit.hip): the setting (cd_set_box_fit; box_on = 0: off) and - grown on demand - the items of a launch
    // (pinned + device), the records (device + pinned mirror), the queue word and the points of cd_box_fit_points; last_box: what
    // cd_get_cluster_box_fits reads, one record per cluster of the last fused call
    int box_on = 0;
    double box_band = CD_BOX_FIT_BAND_DEFAULT;
    DevBuf<BoxItem> d_bfitem; PinBuf<BoxItem> h_bfitem;
    DevBuf<cd_box_fit> d_bfrec; PinBuf<cd_box_fit> h_bfrec;
    DevBuf<int> d_bfqueue;
    DevBuf<float4> d_bfpts;
    KeptRecords<cd_box_fit> last_box;
    std::vector<BoxItem> box_items;        // the items of a fit that has been issued and not collected yet (box_fit.hip)
    std::vector<cd_box_fit> box_rec;       // the records of the last fit, one per cluster / set, complete after its collect
    // the selection (cd_set_box_select; needs box_on): a cluster of a template_slot = -1 call whose record matches a loaded slot's
    // dimensions within the tolerance is registered against that slot alone
    int box_select_on = 0;
    double box_slot_dims[CD_MAX_TEMPLATES][3] = {};
    double box_tolerance = 0.0;
    cd_timing timing;
};

// Where k_ransac_sample's small shuffle map goes when it fills up: SAMPLER_SPILL_PITCH ints per frame, of which the kernel uses
// 2 * SAMPLER_MAP (k_plane.hip asserts that they fit).  The area IS d_head, the bucket heads of the point-graph clustering: the
// plane stage ends before the clustering starts on the context's one stream, stage_cluster fills d_head with 0xff before
// k_cluster_build reads it, and every batch in flight has a context of its own.  Whoever gives d_head another user between the
// plane stage and the clustering has to give the sampler a buffer of its own here.
constexpr int SAMPLER_SPILL_PITCH = CELL_BUCKETS;
inline int* sampler_spill_area(const cd_context* c) { return c->d_head.get(); }

#define HIPCHK(ctx, expr)                                                                                  \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                                   \
            return CD_ERR_DEVICE;                                                                           \
        }                                                                                                   \
    } while (0)

// kernel launches report a bad configuration (grid, LDS size, arguments) through hipGetLastError only: name the kernel
#define LAUNCH(ctx, call)                                                                                     \
    do {                                                                                                      \
        call;                                                                                                 \
        hipError_t e_ = hipGetLastError();                                                                    \
        if (e_ != hipSuccess) {                                                                               \
            snprintf((ctx)->err, sizeof((ctx)->err), "launch failed: %s: %s (%s:%d)", #call, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                                     \
            return CD_ERR_DEVICE;                                                                             \
        }                                                                                                     \
    } while (0)

namespace cd {
// the per-batch read-backs (cd_get_cluster_results, cd_get_frame_cloud, cd_get_cluster_points) describe the last fused call;
// every other compute call reuses the same device buffers
inline void invalidate_last(cd_context* c) {
    c->last_clouds = false;
    c->last_first.clear();
    c->last_surface_ok = false;
    c->last_bboxes_ok = false;
    c->last_outlier_ok = false;
    c->last_prism_ok = false;
    c->last_shapes.invalidate();
    c->last_plane.invalidate();
    c->last_coarse.invalidate();
    c->last_reject.invalidate();
    c->last_recip.invalidate();
    c->last_pair.invalidate();
    c->last_pose.invalidate();
    c->last_box.invalidate();
}

inline int fail(cd_context* c, int code, const char* msg) {
    snprintf(c->err, sizeof(c->err), "%s", msg);
    return code;
}

// ---- chained scans and several contexts on one GPU ---------------------------------------------------------------------------
// A chained scan (crop, radix scatters, voxel heads, cd_extract) waits for tiles with smaller ids.  Since round 4 the ids are
// atomic tickets (take_ticket, common.hpp): the holder of a ticket has started, so a wait can only be for a workgroup that is
// running or done - finite by construction, whatever else shares the GPU.  (Rounds 1-3 took the ids from blockIdx and relied
// on the order in which an XCD starts a grid's workgroups; with several contexts in flight that argument had a hole.)  What is
// left of the old answer to that hole is a safety net that cannot trigger on its own: the waits are still bounded
// (common.hpp), a kernel that gives up reports scan_stalled, and the call is REDONE ALONE - every compute call holds this
// per-device lock shared, the redo exclusively.  CUBOID_FORCE_SCAN_STALL exercises the path.
// The redo must not starve: libstdc++'s shared_mutex is a reader-preferring pthread_rwlock, and with five contexts calling
// back to back some reader nearly always holds it.  So every call first passes a turnstile (a plain mutex, taken and
// released at once); a redo holds the turnstile while it waits for the exclusive lock - new calls queue behind it, the
// calls in flight drain, the redo runs, the queue moves on (tests/test_gpu_readback_guess.py, saturated pipeline).
constexpr int CD_INTERNAL_STALL = -100;   // never leaves the library
constexpr int MAX_DEVICES = 16;

// Admission gate of the whole-cluster ICP launches (CUBOID_ICP_CONCURRENT = K; 0 = none): at most K contexts of a device are
// between the launch of their persistent ICP kernel and its completion.  The launches of several batches otherwise share the
// CUs workgroup by workgroup (processor sharing: five batches submitted together all finish late, together); through the gate
// they run K at a time, first come first served, so the first batches of a burst come back early and their contexts refill
// the pipeline.
struct IcpGate {
    std::mutex mu;
    std::condition_variable cv;
    int inside = 0;
    void enter(int k) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return inside < k; }); ++inside; }
    void leave() { { std::lock_guard<std::mutex> lk(mu); --inside; } cv.notify_one(); }
};
struct GateHold {   // (released on every path out of its scope)
    IcpGate* g = nullptr;
    void enter(IcpGate* gate, int k) { g = gate; g->enter(k); }
    void release() { if (g) { g->leave(); g = nullptr; } }
    ~GateHold() { release(); }
};

// What the contexts of one device share.  ONE object per device and process: the table is defined in context.hip and reached
// through device_shared only - a copy per unit would give each unit locks of its own.
struct DeviceShared {
    std::shared_mutex scan_mu;
    std::mutex turnstile;
    std::atomic<int> calls_in_flight{0};     // one per compute call: counts the contexts at work on the device (k_icp_persist wants the chip to itself)
    std::atomic<int> batches_in_flight{0};   // fused batch calls only: what the launch regime of the whole-cluster ICP kernel looks at
                                             // (a cd_bbox_filter or cd_extract beside a batch must not change the shape of its ICP launch)
    IcpGate icp_gate;
    IcpGate front_gate;   // the same for the front end (crop .. clusters) of the fused batch calls: CUBOID_FRONT_CONCURRENT
};
DeviceShared& device_shared(const cd_context* c);

struct InFlight {   // counts its holder in for its lifetime
    std::atomic<int>& n;
    explicit InFlight(std::atomic<int>& a) : n(a) { n.fetch_add(1); }
    ~InFlight() { n.fetch_sub(1); }
};

// An entry point that runs under the per-device scan lock is `return with_scan_retry(c, [&] { return X_impl(c, ...); });`: the
// null check, the device selection (once: a redo runs on the same thread), then the call under the lock.  The host-only entries,
// the setters and getters, the read-backs, cd_set_template and cd_template_nearest take no lock, as before, and do their own.
template <class Fn>
int with_scan_retry(cd_context* c, Fn&& fn) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    DeviceShared& ds = device_shared(c);
    int st;
    {
        { std::lock_guard<std::mutex> pass(ds.turnstile); }   // held by a pending redo: wait behind it
        std::shared_lock<std::shared_mutex> lk(ds.scan_mu);
        InFlight g(ds.calls_in_flight);
        st = fn();
    }
    if (st != CD_INTERNAL_STALL) return st;
    if (std::getenv("CUBOID_DEBUG")) std::fprintf(stderr, "cuboid_hip: %s - redoing the call with the device to itself\n", c->err);
    c->scan_retries += 1;
    hipStreamSynchronize(c->stream);
    {
        std::lock_guard<std::mutex> hold(ds.turnstile);          // no new call starts until this redo is done
        std::unique_lock<std::shared_mutex> lk(ds.scan_mu);      // ... and the calls in flight have drained
        InFlight g(ds.calls_in_flight);
        st = fn();
    }
    c->timing.scan_retries = 1;
    if (st == CD_INTERNAL_STALL) return fail(c, CD_ERR_DEVICE, "a chained scan stalled twice, the second time with the device to itself");
    return st;
}
}  // namespace cd

// grows a buffer of the context to hold `n` elements (OwnedBuf::ensure: a no-op when it is large enough, otherwise the context's
// stream is synchronised, the old memory freed and new allocated; contents are not kept)
#define GROW(ctx, buf, n) HIPCHK(ctx, (ctx)->buf.ensure((ctx)->stream, (n), #buf))

const int FS_PITCH = (int)(sizeof(FrameState) / sizeof(int));
#define FS_FIELD(ctx, field) ((int*)((char*)(ctx)->d_fs.get() + offsetof(FrameState, field)))

// a stage's zero-fill of one of its scratch arrays - skipped when the fused batch call has zeroed them all in one launch
#define ZERO_FILL(ctx, ptr, bytes)                                                            \
    do {                                                                                      \
        if (!(ctx)->batch_zeroed) HIPCHK(ctx, hipMemsetAsync((ptr), 0, (bytes), (ctx)->stream)); \
    } while (0)

namespace cd {
// consecutive small transfers of a stage collected into one launch (xfer's fallback applies: without copy kernels, or for a
// width that is no multiple of 4, each goes through the runtime's copy as before)
struct XferBatch {
    cd_context* c;
    CopyList L;
    hipError_t err = hipSuccess;
    explicit XferBatch(cd_context* ctx) : c(ctx) { L.n = 0; }
    void add2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, int rows, hipMemcpyKind kind) {
        if (err != hipSuccess || width == 0 || rows <= 0) return;
        if (!c->tun.copy_kernels || (width & 3) || (dpitch & 3) || (spitch & 3)) { err = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, c->stream); return; }
        if (L.n == 8) flush();
        L.seg[L.n++] = CopySeg{(uint32_t*)dst, (const uint32_t*)src, dpitch / 4, spitch / 4, (int)(width / 4), rows};
    }
    void add(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { add2d(dst, bytes, src, bytes, bytes, 1, kind); }
    hipError_t flush() {
        if (L.n > 0 && err == hipSuccess) { launch_copy_list(c->stream, L); err = hipGetLastError(); }
        L.n = 0;
        return err;
    }
};

// depth images of a batch on the device, deprojected into the records d_frames of the fused call (k_depth.hip)
struct DepthJob {
    const cd_depth_camera* cam;
    const uint16_t* depth;
    const uint8_t* color;   // nullptr: no colour
    const cd_color_camera* ccam = nullptr;   // a mapped call (rule C12, k_texture.hip): `color` is ccam->width x ccam->height per frame
};

// ---- context.hip
hipError_t copy_sync(cd_context* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
hipError_t xfer(cd_context* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
int ensure_input(cd_context* c, size_t bytes);
int ensure_clusters(cd_context* c, int ncl, long long points);
int sync_fs(cd_context* c, int F, bool copied = false);   // copied: the caller has put the FrameState read-back on the stream already
int upload_points(cd_context* c, const void* pts, size_t stride, int n, float4* dst);
int check_params(cd_context* c, const cd_params* p);
// ---- icp_plane.hip (rule C17): with the mode on, a loaded template the call would use (slot >= 0: that one; -1: every loaded one)
// that is not a lattice fails the call - to be asked before anything is launched
int check_plane_templates(cd_context* c, int slot);
// ---- icp_reject.hip (rule C19): the mode cannot be combined with rule C17
int check_reject_mode(cd_context* c);
// ---- icp_recip.hip (rule C22): the mode cannot be combined with rule C17 or rule C19
int check_recip_mode(cd_context* c);
// what every ICP entry point asks before it copies or launches anything: check_plane_templates, then check_reject_mode, then
// check_recip_mode (with several wrong the error is the first one's)
inline int check_icp_modes(cd_context* c, int slot) {
    if (int st = check_plane_templates(c, slot)) return st;
    if (int st = check_reject_mode(c)) return st;
    return check_recip_mode(c);
}
int download_records(cd_context* c, const float4* d_pts, int m, size_t stride, int rgb_offset, uint32_t pad3, void* out, size_t staging_skip = 0);
// ---- cuboid_hip.hip
int stage_crop_voxel(cd_context* c, const void* d_in, size_t stride, int N, int F, const cd_params* p, int* rounds_out);
int stage_plane(cd_context* c, int F, const cd_params* p, std::vector<int>& iterations, int* rounds_out, const float* axes = nullptr);
int stage_extract(cd_context* c, int F, const cd_params* p, int gate_mode = -1);
struct ExtractArgs { float thr, z2lo, z2hi; BBoxGate gate; };   // what the S3 kernels take of cd_params (also rule C15's voxel classes)
ExtractArgs extract_args(const cd_params* p, int gate_mode);
int stage_cluster_sync(cd_context* c, int F, const cd_params* p, int max_no);
void set_icp_clusters(cd_context* c, int first, int n, int frame, const int* size, const int* off, int base, int slot);
ShapeFrame template_frame(const cd_context* c, int slot);
// ---- icp_stage.hip
int stage_icp(cd_context* c, int ncl, const cd_params* p, long long* pair_tests, bool device_guesses = false);
void fill_cluster_result(const cd_context* c, int k, const cd_params* p, cd_cluster_result* r);
// rule C18: stage_icp, or - the mode on and a problem of the stage eligible - the coarse stage over the subsamples, the hand-over
// and the stage itself.  h_cl / h_st / h_accf describe the stage's own problems afterwards, h_cstat their stats (mode on).
int stage_icp_levels(cd_context* c, int ncl, const cd_params* p, long long* pair_tests);
// ---- outlier.hip
int stage_outlier(cd_context* c, int F, int max_no, int* map_pitch);
// ---- prism.hip
int stage_prism(cd_context* c, int F, int max_no, int* map_pitch);
int prism_compose_map(cd_context* c, int F, int map_pitch);
// ---- pair_score.hip (rule C21): the fused call's step behind its ICP - every cluster result of the batch against the slot it reports,
// into last_pair (begun here, published by publish_last)
int stage_pair_scores(cd_context* c, int ncl, const std::vector<long long>& orig_off);
// ---- pose_info.hip (rule C23): the fused call's step behind its ICP and rule C21's step - every cluster result of the batch against
// the slot it reports, into last_pose (begun here, published by publish_last)
int stage_pose_info(cd_context* c, int ncl, const std::vector<long long>& orig_off);
// ---- box_fit.hip (rule C24): the fused call's step right after the cluster hand-over - cluster k of frame f (first[f] <= k <
// first[f + 1]) is the size[k] points at d_src0 + orig_off[k], fitted against the frame's plane.  stage_box_fit issues it,
// stage_box_fit_collect ends it: c->box_rec and last_box (begun by the first, published by publish_last)
int stage_box_fit(cd_context* c, int F, const std::vector<int>& first, const std::vector<int>& size, const std::vector<long long>& orig_off);
int stage_box_fit_collect(cd_context* c, int ncl);
// ---- what rules C21 and C23 share on the host: both examine (cluster, template) results after the ICP
struct ResultSpec {   // one result of a launch: its n points at d_src0 + src_off, its T and flag, its slot
    long long src_off;
    int n, slot, accepted;
    const float* T;
};
// rule C8's tau of the range (the setters and the entry points have refused a range that has none)
inline float tau_of(double max_range) {
    float tau = 0.f;
    cd_icp_correspondence_threshold(max_range, &tau, nullptr);
    return tau;
}
// the fused call's results as specs: cluster k's points as extracted, d_src0 + orig_off[k], with what last_clusters[k] reports
inline std::vector<ResultSpec> result_specs(const cd_context* c, int ncl, const std::vector<long long>& orig_off) {
    std::vector<ResultSpec> specs((size_t)ncl);
    for (int k = 0; k < ncl; ++k) {
        const cd_cluster_result& r = c->last_clusters[(size_t)k];
        specs[(size_t)k] = ResultSpec{orig_off[(size_t)k], r.size, r.template_slot, r.accepted, r.T};
    }
    return specs;
}
// the arguments cd_pair_score_points and cd_pose_info_points share, then the rule's own thresholds (ok / what they must be), then
// the capacity - in this order: with several wrong the error is the first one's
inline int check_result_points(cd_context* c, bool has_out, int slot, const void* src_xyz, size_t stride, int n, const float* T, bool thresholds_ok,
                               const char* thresholds_msg) {
    if (!has_out || !T || n < 0 || (n > 0 && !src_xyz) || stride < 12 || (stride & 3) || slot < 0 || slot >= CD_MAX_TEMPLATES) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (!thresholds_ok) return fail(c, CD_ERR_INVALID_ARG, thresholds_msg);
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    return CD_OK;
}
// ---- surface.hip
int ensure_surface(cd_context* c, size_t pitch);
int stage_surface(cd_context* c, int F, int pitch, const std::vector<int>& count, const float* axes, const std::vector<char>& run,
                  int invert, const cd_params* p, cd_surface_frame_result* res, int32_t* status);
void surface_record(int counts[3], float normals[3][4], float mids[3][4], cd_surface_frame_result* r);
int surface_guesses(cd_context* c, int F, const cd_params* p, std::vector<char>* flagged);
int check_color_params(cd_context* c, const cd_color_gate_params* g);
int stage_color(cd_context* c, const uint8_t* d_rgb, int W, int H, int F, const cd_color_gate_params* g);
int color_status(cd_context* c, int F);
// ---- images.hip
void launch_depth_job(hipStream_t s, const DepthJob* dj, int F, float4* out);
int check_depth(cd_context* c, const cd_depth_camera* cam, const void* depth, const void* color, int n_frames);
int check_mapped(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* cc, const void* depth, const void* color, int n_frames);
int upload_depth(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, int n_frames, DepthJob* dj,
                 const cd_color_camera* ccam = nullptr);
}  // namespace cd
