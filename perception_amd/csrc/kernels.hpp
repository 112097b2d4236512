// kernels.hpp - host-callable launchers of every HIP kernel (one .hip file per stage).
#pragma once
#include "common.hpp"

namespace cd {

// k_voxel.hip
void launch_crop_count(hipStream_t s, const void* in, size_t stride, int N, int F, int rgb_off, CropLimits lim, int T,
                       FrameState* fs, int* tile_cnt);
struct ScanJob { int* counts; int* totals; int* mirror; };   // exclusive scan of counts[row][0..T) in place, row totals to totals / mirror[row * pitch]
void launch_scan_tiles(hipStream_t s, int* counts, int rows, int T, int* totals, int total_pitch);
void launch_scan_tiles2(hipStream_t s, const ScanJob& a, const ScanJob& b, int rows, int T, int total_pitch);   // two scans, one launch
void launch_voxel_setup(hipStream_t s, FrameState* fs, int F, float leaf, const uint32_t* ghist, FrameState* mirror);   // (mirror: device-visible host copy of fs, or nullptr)
void launch_crop_fused(hipStream_t s, const void* in, size_t stride, int N, int pitch, int F, int rgb_off, CropLimits lim,
                       int T, float leaf, KeyPack kp, FrameState* fs, int* state, float4* cpt, uint32_t* keys, int* ticket);
void launch_crop_runs(hipStream_t s, const void* in, size_t stride, int N, int pitch, int F, int rgb_off, CropLimits lim,
                      int T, float leaf, KeyPack kp, FrameState* fs, unsigned long long* state, float4* cpt, uint32_t* rkeys,
                      uint32_t* rvals, uint32_t* ghist, int* ticket, int direct);
void launch_crop_compact(hipStream_t s, const void* in, size_t stride, int N, int pitch, int F, int rgb_off, CropLimits lim,
                         int T, float leaf, const FrameState* fs, const int* tile_off, float4* cpt, uint32_t* keys);
void launch_voxel_centroid(hipStream_t s, const uint32_t* keys, const uint32_t* vals, const float4* cpt, int N, int F,
                           int T, int Tact, int rgb_on, FrameState* fs, int* state, float4* vox, int* ticket);
void launch_voxel_centroid_runs(hipStream_t s, const uint32_t* keys, const uint32_t* vals, const float4* cpt, int N, int F,
                                int T, int Tact, int rgb_on, FrameState* fs, int* state, float4* vox, int* ticket, int lanes, int pts_pitch);

void launch_mark_indices(hipStream_t s, const int* idx, int m, int n, int* flag);
struct ZeroRegions { int n; uint32_t* ptr[16]; size_t words[16]; FrameState* fs; int nfs; };   // fs != nullptr: nfs FrameStates set to their initial value (zero, mn = +max) as one more region
void launch_zero_regions(hipStream_t s, const ZeroRegions& r);
struct CopySeg { uint32_t* dst; const uint32_t* src; size_t dpitch_w, spitch_w; int width_w, rows; };   // pitches and width in 4-byte words
struct CopyList { int n; CopySeg seg[8]; };
void launch_copy_list(hipStream_t s, const CopyList& L);
void launch_copy_rows(hipStream_t s, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, int rows);
void launch_passthrough_mark(hipStream_t s, const void* in, size_t stride, int n, int field_off, double lo, double hi, int negative, int* flag);
void launch_select_unmarked(hipStream_t s, const int* flag, int n, int* state, FrameState* fs, int* out, int* ticket);
void launch_gather_records(hipStream_t s, const void* in, int words, const int* idx, int m, void* out);
void launch_pack_records(hipStream_t s, const float4* pts, int m, int words, int rgb_word, uint32_t pad3, void* out);

// k_sort.hip : segmented (per frame) stable LSD radix sort of (key, value) pairs, all passes
constexpr int SORT_MAX_PASSES_HOST = 4;
// (Tact: tiles of SORT_TILE pairs that hold data - k_radix_ghist, k_voxel_runs; Tscat: tiles of SCATTER_TILE pairs - the scatters,
// whose chained-scan state is [passes][F][Tscat][RADIX] ints)
int launch_radix_sort(hipStream_t s, uint32_t* const key[2], uint32_t* const val[2], int N, int F, int Tact, int Tscat, int npass,
                      FrameState* fs, uint32_t* ghist, int* state, KeyPack kp, int* ticket);
// the same sort over RUNS of equal voxel index (k_voxel_runs: 2-3 x fewer elements on organised clouds); tile_state: [F][T] ints
// the scatters alone, over run records whose digit histograms are already in ghist (k_crop_runs): `digits` lists the 8-bit digits
// of the key that vary (ascending); the records are in key[0] / val[0]; Tact counts scatter tiles
int launch_radix_scatter_runs(hipStream_t s, uint32_t* const key[2], uint32_t* const val[2], int N, int F, int Tact, const int* digits, int ndigits,
                              FrameState* fs, const uint32_t* ghist, int* state, int* ticket);
int launch_radix_sort_runs(hipStream_t s, uint32_t* const key[2], uint32_t* const val[2], int N, int F, int T, int Tact, int Tscat, int npass,
                           FrameState* fs, uint32_t* ghist, int* state, int* tile_state, KeyPack kp, int* ticket);

// k_plane.hip
struct FrameRects { const int32_t* rect; int32_t pitch; };   // the gate's rectangle of frame f = rect[f * pitch + 0..3]; rect == nullptr: BBoxGate::rect
void launch_ransac_sample(hipStream_t s, const float4* vox, int N, int F, FrameState* fs, const int* rnd_table,
                          int h_target, const int* active, float4* models, int* valid, int* spill, int spill_pitch);
void launch_ransac_count(hipStream_t s, const float4* vox, int N, int F, int Tact, const FrameState* fs,
                         const float4* models, const int* valid, const int* active, int h0, int h1, float thr, int* counts);
void launch_plane_cov(hipStream_t s, const float4* vox, int N, int F, int Tact, const FrameState* fs, const float4* model,
                      const int* have, float thr, unsigned long long* sums);
void launch_plane_flag_count(hipStream_t s, const float4* vox, int N, int F, int T, int Tact, const FrameState* fs,
                             const float4* model, const int* have, float thr, int negative, int crop2, float z2lo,
                             float z2hi, const BBoxGate& gate, const FrameRects& rects, int* cnt_plane, int* cnt_obj);
void launch_extract_scatter(hipStream_t s, const float4* vox, int N, int F, int T, int Tact, const FrameState* fs,
                            const float4* model, const int* have, float thr, int negative, int crop2, float z2lo,
                            float z2hi, const BBoxGate& gate, const FrameRects& rects, const int* off_plane, const int* off_obj, int* plane_idx,
                            float4* obj);

// k_cluster.hip
void launch_cluster_lds(hipStream_t s, const float4* obj, int N, int F, FrameState* fs, float inv_cell, float r2,
                        int* parent, int* csize, int* rank_of_root);
void launch_cluster_cells(hipStream_t s, const float4* obj, int N, int F, FrameState* fs, float inv_cell, float r2,
                          int* parent, int* csize, int* rank_of_root, float4* sorted);
// The small clustering tier (k_cluster_cells_t, k_cluster.hip): launched instead of k_cluster_lds when no frame of the launch
// has more than CL_TIER_CAP object points.  The bench frames have at most 4306 object points in at most ~800 occupied cells
// (cell edge tol / sqrt(3); 2855 points in 512 cells on average); the table holds 3/4 of its slots.
constexpr int CL_TIER_CAP = 4608;      // object points (nine per thread)
constexpr int CL_TIER_SLOTS = 2048;    // cell table: at most 1536 occupied cells
constexpr int CL_TIER_THREADS = 512;
constexpr int CL_TOP_CAP = 8192;       // k_cluster_lds, the top tier of the one-workgroup kernels with the points in LDS
void launch_cluster_tier(hipStream_t s, const float4* obj, int N, int F, FrameState* fs, float inv_cell, float r2,
                         int* parent, int* csize, int* rank_of_root, float4* sorted);
void launch_cluster_build(hipStream_t s, const float4* obj, int N, int F, int Tact, const FrameState* fs, float inv_cell,
                          int* head, int* next, int* parent, int* csize, int* rank_of_root);
void launch_cluster_hook(hipStream_t s, const float4* obj, int N, int F, int Tact, const FrameState* fs, float inv_cell,
                         float r2, const int* head, const int* next, int* parent);
void launch_cluster_flatten(hipStream_t s, int N, int F, int Tact, const FrameState* fs, int* parent, int* csize);
void launch_cluster_rank(hipStream_t s, int N, int F, FrameState* fs, int enable, int min_sz, int max_sz,
                         const int* parent, const int* csize, int* cand, int* rank_of_root, int* sizes_sorted, FrameState* mirror);
void launch_label_count(hipStream_t s, int N, int F, int T, int Tact, const FrameState* fs, int enable, const int* parent,
                        const int* rank_of_root, int* label, int* tile_cnt, int kbase);
void launch_label_scatter(hipStream_t s, const float4* obj, int N, int F, int T, int Tact, const FrameState* fs,
                          const int* label, const int* tile_off, float4* src0, float4* src, int kbase, const int* koff_tab);

// k_icp.hip (sliced and persistent), k_icp_cluster.hip (whole cluster), k_icp_pipe.hip (pipelined)
// What every ICP launch takes, in three blocks that icp_stage.hip fills once per stage; each launcher picks what its kernel reads.
struct IcpProblems {   // the problem set: device pointers, or (k_icp_lat's direct mode) the pinned host arrays
    const int* order; const IcpCluster* cl; IcpState* st; unsigned long long* accf;
};
struct IcpTemplates {   // the template tables: points + per-64-run boxes in cell order (tpl, tlo, thi) and in k-d patch order (tplk, tlok, thik)
    const float4 *tpl, *tplk, *tlo, *thi, *tlok, *thik;
    const unsigned short* kdmap; const IcpGrid* grids; const IcpSuper* supers; const unsigned short* tcell; const IcpLattice* lats;
};
struct IcpScratch { float4* src; const float4* src0; int* nn; float* d2; unsigned long long* acc; int* queue; };
// ONE lane pops the next live problem of a launch's queue (order: largest first), skipping those the host pre-marked (too few
// points / no template).  Returns its index with c = its description, or -1: nothing left.
__device__ __forceinline__ int icp_pop_live(int* queue, int nitems, const int* order, const IcpCluster* cl, const IcpState* st, IcpCluster& c) {
    for (;;) {
        const int item = atomicAdd(queue, 1);
        if (item >= nitems) return -1;
        const int k = order[item];
        if (st[2 * (size_t)k].done) continue;
        c = cl[k];
        return k;
    }
}
// (the sliced, persistent and fitness kernels search the k-d patch order with its boxes)
void launch_icp_iter(hipStream_t s, int it, int n_work, int ncl, const IcpWork* work, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S,
                     int qslice, int n_cu, IcpParams prm, const IcpBound& bnd);
void launch_icp_persist(hipStream_t s, int n_work, int n_wg, int max_it, const IcpWork* work, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S,
                        int qslice, unsigned* bar, int* abort_flag, int n_open, int* closed, IcpParams prm, const IcpBound& bnd);
void launch_icp_fitness(hipStream_t s, int n_work, const IcpWork* work, const IcpProblems& P, int parity, const IcpTemplates& T, const IcpScratch& S, int qslice);

void launch_icp_apply_guess(hipStream_t s, int ncl, int max_n, const IcpCluster* cl, const float* guesses, int per_frame,
                            const float4* src0, float4* src);
// (k_icp_pipe: the cell order with the k-d boxes; k_icp_pipe_big: both orders with the k-d boxes; k_icp_cluster: the cell order with its boxes)
void launch_icp_pipe(hipStream_t s, int ncl, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, int n_wg, const int* wgtab, IcpParams prm, const IcpBound& bnd);
void launch_icp_pipe_big(hipStream_t s, int ncl, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, int n_wg, const int* wgtab, IcpParams prm, const IcpBound& bnd);
void launch_icp_cluster(hipStream_t s, int ncl, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, int n_cu, IcpParams prm, const IcpBound& bnd);

// k_icp_lat.hip : templates that are unions of axis-aligned lattices (IcpLattice) - closed-form nearest neighbour
void launch_icp_lat(hipStream_t s, int nitems, int cpw, int wpc, int n_wg, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S,
                    unsigned long long* busy, unsigned long long* busy_out, IcpParams prm, const IcpBound& bnd);
void launch_lat_nn(hipStream_t s, const IcpLattice* lat, const float4* q, int n, int* out_idx, float* out_d2);

// k_icp_plane.hip : rule C17, the plane-weighted ICP step for lattice templates (icp_plane_math.hpp: PlaneStats, PlaneParams);
// n_wg workgroups take the nitems problems of P.order from S.queue[0], one at a time
struct PlaneStats;
struct PlaneParams;
void launch_icp_plane(hipStream_t s, int nitems, int n_wg, const IcpProblems& P, PlaneStats* pstat, const IcpTemplates& T, const IcpScratch& S,
                      IcpParams prm, const IcpBound& bnd, const PlaneParams& pp);

// k_icp_coarse.hip : rule C18, the subsample before the coarse stage and the hand-over inside the fine stage's set-up
// (icp_coarse_plan.hpp: CoarseGather, CoarseHand, CoarseStats)
struct CoarseGather;
struct CoarseHand;
struct CoarseStats;
void launch_icp_coarse_gather(hipStream_t s, int n_coarse_problems, int max_n_coarse, const CoarseGather* tab, float4* src0, float4* src);
void launch_icp_coarse_handover(hipStream_t s, int ncl, const CoarseHand* hand, const IcpState* cst, const unsigned long long* caccf, IcpState* st,
                                float* guess, CoarseStats* stats);

// k_icp_reject.hip : rule C19, median-distance correspondence rejection (icp_reject_math.hpp: RejectStats) - behind k_icp_iter<true>(it)
// of the sliced loop: the sums and count of iteration slot it % 3 of every live, unfinished problem become those of the kept
// correspondences (S.nn / S.d2 as the iteration kernel left them, T.tplk); bnd.d2_max = +inf without rule C8's bound
struct RejectStats;
void launch_icp_reject(hipStream_t s, int it, int ncl, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, const IcpBound& bnd, double factor,
                       RejectStats* rstat);

// k_icp_recip.hip : rule C22, reciprocal correspondences (icp_recip_math.hpp: RecipStats) - behind k_icp_iter<true>(it) of the sliced
// loop, as k_icp_reject: the reverse test of every live, unfinished problem's points (query ranges of a problem over
// blockIdx.y; max_n: the largest problem) leaves one flag per point in `keep` (indexed as S.src), then the slot's sums and count
// become those of the flagged correspondences; bnd.d2_max = +inf without rule C8's bound
struct RecipStats;
void launch_icp_recip(hipStream_t s, int it, int ncl, int max_n, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, const IcpBound& bnd,
                      uint8_t* keep, RecipStats* rstat);

// k_depth.hip : n_frames tightly packed 16UC1 depth images (+ rgb8 colour, or nullptr) -> width * height * n_frames float4
// records x y z rgb (canonical rule C7)
struct DeprojectParams {
    int width, height;
    float fx, fy, cx, cy, depth_scale;
    uint32_t stepu, stepv;   // BLOCK pixels further on: columns, rows (modulo the frame)
    size_t total;            // pixels of the batch
};
void launch_deproject(hipStream_t s, const uint16_t* depth, const uint8_t* color, int width, int height, int n_frames, float fx,
                      float fy, float cx, float cy, float depth_scale, float4* out);

// k_texture.hip : rule C12, unregistered depth + colour images -> the coloured organized cloud (texture_math.hpp: TextureParams)
struct TextureParams;
void launch_texture_map(hipStream_t s, const uint16_t* depth, const uint8_t* color, int width, int height, int n_frames,
                        const TextureParams& tp, float4* out);

// k_surface.hip : the batched surface-normal estimation's cloud load and plane midpoints (rule C6 sums)
void launch_surface_load(hipStream_t s, const void* in, size_t stride, size_t fpitch, const int* count, int count_pitch, int pitch,
                         int max_count, int F, float4* out);
void launch_surface_centroid(hipStream_t s, const float4* pts, int pitch, int F, const FrameState* fs, const float4* model,
                             const int* have, float thr, int invert, float4* out, int out_pitch);


// k_shape.hip : rule C13, one workgroup per point set -> one ShapeFrame (= cd_shape_frame); fused form: + the ICP guess of the set
struct ShapeFrame;
void launch_shape_frames(hipStream_t s, int n_sets, const IcpCluster* cl, const float4* pts, ShapeFrame* rec, const ShapeFrame* tframe,
                         float* guess, IcpState* st);

// k_color.hip : rule C10, one workgroup per rgb8 image -> one ColorRecord (= cd_color_bbox) per frame
constexpr int COLOR_BLOCK = 1024;
constexpr int COLOR_LDS_WORDS = 30720;   // both halves of a frame's packed mask, 120 KiB
struct ColorGate { int32_t h_lo_max, h_hi_min, s_min, v_min, margin; };
struct ColorRecord { int32_t rect[4], found, area2, n_components, n_mask; };
bool color_fits_lds(int W, int H);
// tables: sdiv[256] then hdiv[256]; gmask: nullptr (the mask fits LDS) or 2 * ceil(W / 32) * H words per frame; labels:
// label_pitch >= W * H ints per frame; status: CD_OK / CD_ERR_CAPACITY per frame
void launch_color_bbox(hipStream_t s, const uint8_t* rgb, int W, int H, int F, const ColorGate& prm, const int* tables,
                       uint32_t* gmask, int* labels, size_t label_pitch, ColorRecord* out, int* status);

// k_overlay.hip : rule C11, the projected boxes of draw_bbox.py drawn into tightly packed rgb8 images in place
struct OverlayParams { double M[12]; double dims[3]; };   // M = P * E (row-major 3x4), the box's length / width / height
struct OverlayBox { int32_t corners[16], drawn, reserved[3]; };   // = cd_overlay_box
// poses: F * B row-major 4x4 doubles, box b of frame f at (f * B + b) * 16; n_boxes[f] <= B of them exist; out: F * B records
void launch_overlay_project(hipStream_t s, const double* poses, const int32_t* n_boxes, int B, int F, const OverlayParams& op, OverlayBox* out);
// img: F images of W * H * 3 bytes, W, H <= 8192; thickness 1 .. 64; boxes: the F * B records of launch_overlay_project
void launch_overlay_raster(hipStream_t s, uint8_t* img, int W, int H, int B, int F, int thickness, const uint8_t rgb[3], const OverlayBox* boxes);

// k_verify.hip : rule C14, one workgroup per (frame, slot) -> one VerifyRecord (= cd_verify_box without score and passed)
struct VerifyCam;
struct VerifyJob { double pose[16]; double dims[3]; };   // what crosses the bus per box: 152 bytes
struct VerifyRecord { int32_t verified, passed, n_hit, n_agree, n_through, n_occluded, n_invalid, reserved; long long agree_abs_um; double score; };
// depth: F images of cam.width * cam.height uint16; jobs: F * B, box b of frame f at f * B + b; n_boxes[f] <= B of them exist;
// out: F * B records (all zero for the slots that do not exist)
void launch_verify_boxes(hipStream_t s, const uint16_t* depth, const VerifyCam& cam, double tau, const VerifyJob* jobs, const int32_t* n_boxes,
                         int B, int F, VerifyRecord* out);

// k_labels.hip : rule C15, the label of every input record of the last fused call, and the tint of label images
// step 1: voxel v's key, in the order of d_vox, from the frame's sorted keys (rows of N; n_runs of them when by_runs, else n_c) -> vkey[f * vpitch + v]
void launch_label_voxel_keys(hipStream_t s, const uint32_t* keys, int N, int F, const FrameState* fs, int by_runs, uint32_t* vkey, int vpitch);
// step 2: voxel v's class (CD_LABEL_PLANE / OBJECT / GATED / CLUSTER0 + r) from the call's plane index list, the S3 predicate and
// the cluster labels -> vclass[f * vpitch + v].  omap.map != nullptr: the call filtered its object clouds (rule C16) - a voxel
// that S3 moved and the filter removed stays CD_LABEL_GATED, the others index the labels through the map
struct OutlierRecord;
struct OutlierMap { const int* map; const OutlierRecord* rec; int pitch; };   // map[f * pitch + r]: index in the filtered cloud, or -1
void launch_label_voxel_classes(hipStream_t s, const float4* vox, int N, int F, const FrameState* fs, const float4* model, const int* have,
                                float thr, int negative, int crop2, float z2lo, float z2hi, const BBoxGate& gate, const FrameRects& rects,
                                const int* plane_idx, const int* label, uint8_t* vclass, int vpitch, const OutlierMap& omap);
// step 3: the batch as one linear stream of F * P records (depth == nullptr: `stride` bytes each, x y z first) or pixels (rule C7)
struct LabelPointsParams {
    CropLimits lim;
    float inv_leaf;
    int32_t packed;          // the keys are k_crop_runs' bit fields (kp), else PCL's idx
    KeyPack kp;
    uint32_t P;              // records / pixels per frame
    int32_t F, vpitch;
    uint32_t width;          // depth form
    float fx, fy, cx, cy, depth_scale;
};
void launch_label_points(hipStream_t s, const void* records, size_t stride, const uint16_t* depth, const LabelPointsParams& lp,
                         const FrameState* fs, const uint32_t* vkey, const uint8_t* vclass, uint8_t* out);
struct LabelPalette { uint32_t rgba[256]; };   // = cd_label_palette: byte 0 r, 1 g, 2 b, 3 alpha
void launch_tint_labels(hipStream_t s, uint8_t* rgb, const uint8_t* labels, size_t pixels, const LabelPalette& pal);

// k_outlier.hip : rule C16, statistical outlier removal on F rows of N points (row f holds fs[f].n_o of them, max_n at the most)
// step 1: dist_i of every point -> dist[f * dpitch + i] (0 for a non-finite point and in a row of no more than mean_k finite points)
void launch_outlier_knn(hipStream_t s, const float4* pts, int N, int F, int max_n, const FrameState* fs, int mean_k, float* dist, int dpitch);
// step 2: the row's statistics -> rec[f]; the kept points in order -> out[f * N ..] (nullptr: none), their indices ->
// kept_idx[f * N ..] (nullptr: none), every point's index in the filtered row or -1 -> map[f * mpitch + i]; fs[f].n_o (and the
// mirror's, when given) becomes the kept count
void launch_outlier_select(hipStream_t s, const float4* pts, int N, int F, FrameState* fs, FrameState* mirror, const float* dist, int dpitch,
                           int mean_k, double std_mul, int negative, float4* out, int* map, int mpitch, int* kept_idx, OutlierRecord* rec);

// k_prism.hip : rule C20, the table prism on F rows of N points.  Row f: its plane inliers are the points plane_pts[f * N +
// plane_idx[f * N + i]], i < fs[f].n_plane (plane_idx == nullptr: the first n_plane points of the row); model[f] the plane, have[f]
// whether it has one (nullptr: every row has); its cloud pts[f * N ..] of fs[f].n_o points.  scratch: N (u, v) pairs per row.
// out / kept_idx / map / mirror as launch_outlier_select; rec[f] the row's record, lrec[f] the same counts in the form the label
// calls read beside the map, hull[f * 2 * CD_PRISM_MAX_HULL ..] the row's hull vertices (nullptr: none).
struct PrismRecord;
struct PrismArgs {
    const float4* plane_pts; const int* plane_idx; const float4* model; const int* have;
    const float4* pts; int N;
    FrameState* fs; FrameState* mirror;
    double hmin, hmax;
    int2* scratch;
    float4* out; int* map; int mpitch; int* kept_idx;
    PrismRecord* rec; OutlierRecord* lrec; int32_t* hull;
};
void launch_prism(hipStream_t s, int F, const PrismArgs& a);
// pmap[f * pitch + e] <- omap[f * pitch + pmap[f * pitch + e]] (or -1), e < lrec[f].n_before: the prism's map followed by the filter's
void launch_prism_compose_map(hipStream_t s, int F, int* pmap, const OutlierRecord* lrec, const int* omap, int pitch);

// k_pair_score.hip : rule C21, the two-way registration score (pair_score_math.hpp).  A job is one direction of one pair: q_src != 0:
// the queries are the nq points src[q_off ..] under T and the targets the ng points tpl[g_off ..]; q_src == 0: the queries are
// tpl[q_off ..] and the targets src[g_off ..] under T.  An item is the queries q0 .. q0 + qn (1 <= qn <= PS_CHUNK) of a job.
// n_wg workgroups draw the items from *queue (zero before the launch) and add into acc[pair * PAIR_ACC_PITCH ..] (zero before it).
constexpr int PS_THREADS = 256, PS_ROWS = 4, PS_CHUNK = 1024, PS_TILE = 1024;
struct PairJob { int32_t q_off, nq, g_off, ng, q_src, pair, pad[2]; float T[12]; };
struct PairItem { int32_t job, q0, qn, pad; };
void launch_pair_score(hipStream_t s, int n_items, int n_wg, const PairJob* jobs, const PairItem* items, const float4* src, const float4* tpl, float tau,
                       unsigned long long* acc, int* queue);

// k_pose_info.hip : rule C23, the pose information of (cluster, lattice template) results (pose_info_math.hpp).  An item is one
// result: its n >= 1 points src0[src_off ..], T, the slot (a lattice: lats[slot].nface > 0) with its centre and length, the
// result's accepted flag and the record it fills, out[pair].  n_wg workgroups draw the items from *queue (zero before the launch).
struct PoseItem { int32_t src_off, n, slot, accepted, pair, pad[3]; float T[12]; float c0[3]; float pad2; double length; };
void launch_pose_info(hipStream_t s, int nitems, int n_wg, const PoseItem* items, const IcpLattice* lats, const float4* src0, float tau, double min_support,
                      cd_pose_info* out, int* queue);

// k_box_fit.hip : rule C24, the box fit of clusters (box_fit_math.hpp, which defines the item).  An item is one cluster: its n points
// pts[src_off ..], its frame's oriented plane and basis, the band and the record it fills, out[rec].  n_wg workgroups draw the items
// from *queue (zero before the launch).
struct BoxItem;
void launch_box_fit(hipStream_t s, int nitems, int n_wg, const BoxItem* items, const float4* pts, cd_box_fit* out, int* queue);

}  // namespace cd
