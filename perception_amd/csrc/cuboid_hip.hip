// cuboid_hip.hip - context, batch pipeline driver and the C-ABI of include/cuboid_hip.h.
//
// The whole chain runs on one HIP stream with every intermediate resident in HBM
// (frame-major arrays, pitch = points per frame).  The host only (a) sizes launches from a
// handful of per-frame scalars mirrored through pinned memory, (b) replays PCL's sequential
// RANSAC stop rule over the batched inlier counts, (c) solves the 3x3 plane-refit eigenproblem
// and (d) polls ICP completion.  There is no CPU compute fallback of any stage.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <atomic>
#include <mutex>
#include <shared_mutex>
#include <condition_variable>
#include <random>
#include <vector>

#include "device_buffer.hpp"
#include "host_math.hpp"
#include "kernels.hpp"
#include "overlay_math.hpp"
#include "verify_math.hpp"
#include "shape_frame_math.hpp"
#include "template_prep.hpp"
#include "texture_math.hpp"

using namespace cd;

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
    bool crop_two_pass = false;   // CUBOID_CROP_TWO_PASS=1: always the two-pass crop
    int icp_persist = 1;          // CUBOID_ICP_PERSIST=0: the sliced driver always in its multi-launch form; 2: the persistent
                                  // launch starts with its abort flag raised (tests the hand-over to the multi-launch form)
    // point buffers (float4 = x,y,z,rgb bits)
    DevBuf<float4> d_cpt, d_vox, d_obj, d_src0, d_src;
    DevBuf<uint32_t> d_key[2], d_val[2], d_ghist;
    DevBuf<int> d_sstate;   // chained-scan state of the radix passes, [pass][F][scatter tiles][256]
    DevBuf<unsigned long long> d_tile64;   // chained-scan state of k_crop_runs: (points, runs) per tile, [F][T]
    bool crop_runs = true;      // CUBOID_CROP_RUNS=0: the crop writes per-point keys and k_voxel_runs finds the runs (rounds 2-3)
    DevBuf<int> d_ticket;   // ticket counters, one per frame (TICKET_PITCH ints apart), of the kernels that scan over tiles (take_ticket, common.hpp): zero between launches
    // RANSAC
    DevBuf<int> d_rnd, d_valid, d_counts, d_active, d_have;
    PinBuf<int> h_valid, h_counts, h_active, h_have;
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
    int don_idle = 0, don_fault = 0;                              // CUBOID_ICP_DON_IDLE / CUBOID_ICP_DON_FAULT: tests of the hand-over path (IcpParams::don_idle / don_fault)
    int icp_donate = -1;                                          // CUBOID_ICP_DONATE: -1 auto (a call alone on the device), 0 never, 1 always
    DevBuf<int> d_wgtab;                                          // k_icp_pipe: {first item, end item, queue} per workgroup
    PinBuf<int> h_wgtab;                                          // its pinned staging copy (3 * 1024 ints)
    PinBuf<int> h_ctl;                                            // pinned: control words of k_icp_persist going up [0..7], coming back [8]
    std::vector<IcpState> st_init;                                // initial ICP states of a persistent launch (kept in case it gives up)
    int force_stall = 0;                                          // CUBOID_FORCE_SCAN_STALL=n: the next n chained-scan checks report a stall (tests the retry)
    int scan_retries = 0;                                         // calls of this context that were redone because a chained scan stalled
    int persist_gave_up = 0;                                      // persistent launches of this context that handed over to the multi-launch loop
    int n_cu = 256;
    int icp_mode = 0;                                             // 0 auto, 1 sliced multi-launch, 2 whole-cluster kernel
    int icp_max_wg = 0;                                           // > 0: cap on the persistent ICP grid (CUBOID_ICP_MAX_WG; tests force slot refills with it)
    int icp_cpw = 0;                                              // CUBOID_ICP_CPW: clusters per workgroup a persistent ICP launch is sized for (0: by regime, icp_run_whole)
    bool fs_initialised = false;                                  // the device FrameStates hold their initial value (set by the zero launch of a fused batch call)
    int icp_direct = 1;                                           // CUBOID_ICP_DIRECT=0: an all-lattice ICP stage uploads its lists and reads its results back by copy launches
    int mirror_reads = 1;                                         // CUBOID_MIRROR_READS=0: active flags and chosen plane models are uploaded before the kernels that read them
    int mirror_writes = 1;                                        // CUBOID_MIRROR_WRITES=0: every host read-back of the FrameState array is a copy launch again
    int cluster_cells = 1;                                        // CUBOID_CLUSTER_CELLS=0: frames above 8192 object points straight to the point-graph kernels (rounds 1-5)
    int crop_direct = 1;                                          // CUBOID_CROP_DIRECT=0: the crop always copies the kept points (rounds 1-5)
    int centroid_lanes = 1;                                       // CUBOID_CENTROID_LANES=0: the quad-per-voxel centroid kernel (rounds 3-5) instead of a lane per voxel
    bool voxel_runs = true;                                       // CUBOID_VOXEL_RUNS=0: S1 sorts the cropped points instead of their runs of equal voxel index
    int icp_slots = 0;                                            // CUBOID_ICP_SLOTS: clusters in flight per workgroup, 1 .. CD_PIPE_SLOTS (0: by regime)
    int icp_big_weight = 0;                                       // workgroup share of a template in global memory, per point (CUBOID_ICP_BIG_WEIGHT; 0 = by the launch's regime, measured on config 5)
    DevBuf<int> d_order; PinBuf<int> h_order;                     // clusters, largest first
    int tpl_cap = 0, tpl_used = 0;
    std::shared_ptr<const cd::PreparedTemplate> tpl_prep[CD_MAX_TEMPLATES];   // host copies (shared across contexts)
    int tpl_off[CD_MAX_TEMPLATES] = {0}, tpl_m[CD_MAX_TEMPLATES] = {0};
    bool tpl_gridded[CD_MAX_TEMPLATES] = {false};                // slot has a cell start table
    bool tpl_big[CD_MAX_TEMPLATES] = {false};                    // slot does not fit LDS but has what k_icp_pipe_big needs (cell table, k-d map, superpatches)
    DevBuf<IcpSuper> d_super;                                     // per template slot
    DevBuf<IcpLattice> d_lat;                                     // per template slot: axis tables and faces of a lattice template (nface = 0: none)
    int tpl_faces[CD_MAX_TEMPLATES] = {0};                        // faces of the slot's lattice (0: the generic searches take it)
    int icp_lattice = 1;                                          // CUBOID_ICP_LATTICE=0: lattice templates take the generic searches too (A/B, fallback tests)
    int zero_once = 1;                                            // CUBOID_ZERO_ONCE=0: every stage of a fused batch call fills its scratch arrays itself (A/B)
    int copy_kernels = 1;                                         // CUBOID_COPY_KERNELS=0: the small pinned <-> device transfers go through hipMemcpyAsync (SDMA) again
    int lat_shape[3] = {0, 0, 0};                                 // CUBOID_LAT_SHAPE=cpw,wpc[,per_slot]: clusters per workgroup, waves per cluster, clusters per slot of k_icp_lat (0: by regime)
    int front_concurrent = 0;                                     // CUBOID_FRONT_CONCURRENT: at most that many fused batch calls of the device between crop and clusters (0 = no gate)
    int icp_concurrent = 0;                                       // CUBOID_ICP_CONCURRENT: admission gate of the whole-cluster ICP launches (0 = none)
    int icp_lowprio = 1;                                          // CUBOID_ICP_LOWPRIO: 0 never, 1 the launches of a mixed-template batch (measured: config 5 +30 %), 2 every
                                                                  // persistent ICP launch (config 3: -1 %)
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
    std::vector<cd_shape_frame> last_shapes;                      // cd_get_cluster_shape_frames: one per cluster of the last fused call, frame-major
    bool last_shapes_ok = false;
    DevBuf<IcpState> d_st; PinBuf<IcpState> h_st;
    DevBuf<unsigned long long> d_acc, d_accf; PinBuf<unsigned long long> h_accf;
    cd_timing timing;
};

namespace {

#define HIPCHK(ctx, expr)                                                                                   \
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

// the per-batch read-backs (cd_get_cluster_results, cd_get_frame_cloud, cd_get_cluster_points) describe the last fused call;
// every other compute call reuses the same device buffers
void invalidate_last(cd_context* c) {
    c->last_clouds = false;
    c->last_first.clear();
    c->last_surface_ok = false;
    c->last_bboxes_ok = false;
    c->last_shapes_ok = false;
}

int fail(cd_context* c, int code, const char* msg) {
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
std::shared_mutex g_scan_mu[MAX_DEVICES];
std::mutex g_turnstile[MAX_DEVICES];
std::atomic<int> g_calls_in_flight[MAX_DEVICES];

std::atomic<int> g_batches_in_flight[MAX_DEVICES];   // fused batch calls only: what the launch regime of the whole-cluster ICP kernel looks at
struct BatchGuard {  // (a cd_bbox_filter or cd_extract beside a batch must not change the shape of its ICP launch)
    int dev;
    explicit BatchGuard(int d) : dev(d & (MAX_DEVICES - 1)) { g_batches_in_flight[dev].fetch_add(1); }
    ~BatchGuard() { g_batches_in_flight[dev].fetch_sub(1); }
};
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
IcpGate g_icp_gate[MAX_DEVICES];
IcpGate g_front_gate[MAX_DEVICES];   // the same for the front end (crop .. clusters) of the fused batch calls: CUBOID_FRONT_CONCURRENT
struct GateHold {   // (released on every path out of its scope)
    IcpGate* g = nullptr;
    void enter(IcpGate* gate, int k) { g = gate; g->enter(k); }
    void release() { if (g) { g->leave(); g = nullptr; } }
    ~GateHold() { release(); }
};
struct CallGuard {   // one per compute call: counts the contexts at work on the device (k_icp_persist wants the chip to itself)
    int dev;
    explicit CallGuard(int d) : dev(d & (MAX_DEVICES - 1)) { g_calls_in_flight[dev].fetch_add(1); }
    ~CallGuard() { g_calls_in_flight[dev].fetch_sub(1); }
};

template <class Fn>
int with_scan_retry(cd_context* c, Fn&& fn) {
    const int dev = c->device & (MAX_DEVICES - 1);
    int st;
    {
        { std::lock_guard<std::mutex> pass(g_turnstile[dev]); }   // held by a pending redo: wait behind it
        std::shared_lock<std::shared_mutex> lk(g_scan_mu[dev]);
        CallGuard g(dev);
        st = fn();
    }
    if (st != CD_INTERNAL_STALL) return st;
    if (std::getenv("CUBOID_DEBUG")) std::fprintf(stderr, "cuboid_hip: %s - redoing the call with the device to itself\n", c->err);
    c->scan_retries += 1;
    hipStreamSynchronize(c->stream);
    {
        std::lock_guard<std::mutex> hold(g_turnstile[dev]);          // no new call starts until this redo is done
        std::unique_lock<std::shared_mutex> lk(g_scan_mu[dev]);      // ... and the calls in flight have drained
        CallGuard g(dev);
        st = fn();
    }
    c->timing.scan_retries = 1;
    if (st == CD_INTERNAL_STALL) return fail(c, CD_ERR_DEVICE, "a chained scan stalled twice, the second time with the device to itself");
    return st;
}

// grows a buffer of the context to hold `n` elements (OwnedBuf::ensure: a no-op when it is large enough, otherwise the context's
// stream is synchronised, the old memory freed and new allocated; contents are not kept)
#define GROW(ctx, buf, n) HIPCHK(ctx, (ctx)->buf.ensure((ctx)->stream, (n), #buf))

const int FS_PITCH = (int)(sizeof(FrameState) / sizeof(int));
#define FS_FIELD(ctx, field) ((int*)((char*)(ctx)->d_fs.get() + offsetof(FrameState, field)))

// blocking copy ordered on the context's own (non-blocking) stream: the NULL stream gives no ordering against it
static hipError_t copy_sync(cd_context* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}

// a small transfer between a PINNED host mirror of the context and device memory, as a kernel on the context's stream
// (launch_copy_rows, k_plane.hip: why not hipMemcpyAsync).  bytes: a multiple of 4.  CUBOID_COPY_KERNELS=0: hipMemcpyAsync (A/B).
static hipError_t xfer(cd_context* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!c->copy_kernels || (bytes & 3)) return hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    launch_copy_rows(c->stream, dst, bytes, src, bytes, bytes, 1);
    return hipGetLastError();
}
static hipError_t xfer2d(cd_context* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, int rows, hipMemcpyKind kind) {
    if (!c->copy_kernels || (width & 3) || (dpitch & 3) || (spitch & 3)) return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, c->stream);
    launch_copy_rows(c->stream, dst, dpitch, src, spitch, width, rows);
    return hipGetLastError();
}

// a stage's zero-fill of one of its scratch arrays - skipped when the fused batch call has zeroed them all in one launch
#define ZERO_FILL(ctx, ptr, bytes)                                                            \
    do {                                                                                      \
        if (!(ctx)->batch_zeroed) HIPCHK(ctx, hipMemsetAsync((ptr), 0, (bytes), (ctx)->stream)); \
    } while (0)

// consecutive small transfers of a stage collected into one launch (xfer's fallback applies: without copy kernels, or for a
// width that is no multiple of 4, each goes through the runtime's copy as before)
struct XferBatch {
    cd_context* c;
    CopyList L;
    hipError_t err = hipSuccess;
    explicit XferBatch(cd_context* ctx) : c(ctx) { L.n = 0; }
    void add2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, int rows, hipMemcpyKind kind) {
        if (err != hipSuccess || width == 0 || rows <= 0) return;
        if (!c->copy_kernels || (width & 3) || (dpitch & 3) || (spitch & 3)) { err = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, c->stream); return; }
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

int ensure_input(cd_context* c, size_t bytes) {
    GROW(c, d_in, bytes);
    return CD_OK;
}

// cluster-indexed ICP arrays: sized for F * KICP problems at cd_create, re-allocated when a batch holds more
// (frames with more than KICP clusters) - no cluster is dropped
int ensure_clusters(cd_context* c, int ncl, long long points) {
    const long long work_need = points / 64 + (long long)ncl + 16;
    if (ncl <= c->cl_cap && work_need <= c->work_cap) return CD_OK;
    if (work_need > 0x7fffffffll) return fail(c, CD_ERR_CAPACITY, "ICP work list exceeds 2^31 items");
    c->batch_zeroed = false;   // (new arrays: stage_icp fills them itself)
    // never shrink: the per-stage entry points (cd_icp) rely on the capacity cd_create gave them
    const size_t n = (size_t)std::max(std::max(ncl, c->F * KICP) + ncl / 4, c->cl_cap), w = (size_t)std::max<long long>(work_need + work_need / 4, c->work_cap);
    c->cl_cap = 0; c->work_cap = 0;
    GROW(c, d_cl, n); GROW(c, h_cl, n);
    GROW(c, d_order, n); GROW(c, h_order, n);
    GROW(c, d_work, w); GROW(c, h_work, w);
    GROW(c, d_work2, w); GROW(c, h_work2, w);
    GROW(c, d_st, n * 2); GROW(c, h_st, n * 2);
    GROW(c, d_acc, n * 48); GROW(c, d_accf, n + 1); GROW(c, h_accf, n + 1);   // (+ 1: k_icp_lat's wave-time word)
    c->cl_cap = (int)n;
    c->work_cap = (int)w;
    return CD_OK;
}

int sync_fs(cd_context* c, int F, bool copied = false) {   // copied: the caller has put the FrameState read-back on the stream already
    if (!copied) HIPCHK(c, xfer(c, c->h_fs, c->d_fs, sizeof(FrameState) * F, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < F; ++f)
        if (c->h_fs[f].scan_stalled) return fail(c, CD_INTERNAL_STALL, "a chained scan stalled (workgroups of a grid were not started in id order)");
    if (c->force_stall > 0) { c->force_stall -= 1; return fail(c, CD_INTERNAL_STALL, "a chained scan stalled (forced: CUBOID_FORCE_SCAN_STALL)"); }
    return CD_OK;
}

// ---- stage drivers (device-resident in/out; F frames) ------------------------------------

// S0+S1.  in: F*N records of `stride` bytes on the device.  out: d_vox / fs.n_v
int stage_crop_voxel(cd_context* c, const void* d_in, size_t stride, int N, int F, const cd_params* p, int* rounds_out) {
    const int T = c->T;
    CropLimits lim;
    lim.zlo = hm::fold_ge(p->crop_z_min);
    lim.zhi = hm::fold_le(p->crop_z_max);
    lim.xlo = hm::fold_ge(p->crop_x_min);
    lim.xhi = hm::fold_le(p->crop_x_max);
    const int rgb_off = (p->rgb_offset >= 0 && (size_t)p->rgb_offset + 4 <= stride) ? p->rgb_offset : -1;
    // FrameState init: status 0, mn = +max, mx = 0 (ordered-uint encoding)
    for (int f = 0; f < F; ++f) {
        FrameState& s = c->h_fs[f];
        std::memset(&s, 0, sizeof(s));
        for (int a = 0; a < 3; ++a) { s.mn[a] = 0xffffffffu; s.mx[a] = 0u; }
    }
    // Single pass (one read of the input) when the crop limits bound the x and z cell indices tightly enough to leave the
    // unbounded y index a wide bit field; a frame whose y does not fit anyway sends the batch through the two-pass path.
    KeyPack kp;
    std::memset(&kp, 0, sizeof(kp));
    {
        const float inv = 1.0f / p->leaf_size;
        const float fl[4] = {std::floor(lim.xlo * inv), std::floor(lim.xhi * inv), std::floor(lim.zlo * inv), std::floor(lim.zhi * inv)};
        bool ok = !c->crop_two_pass;
        for (float v : fl) ok = ok && std::fabs(v) < 1.0e9f;
        if (ok && fl[1] >= fl[0] && fl[3] >= fl[2]) {
            const long long ri = (long long)fl[1] - (long long)fl[0] + 1, rk = (long long)fl[3] - (long long)fl[2] + 1;
            int bi = 1, bk = 1;
            while ((1ll << bi) < ri) ++bi;
            while ((1ll << bk) < rk) ++bk;
            if (bi + bk <= 20) {
                kp.enabled = 1;
                kp.bi = bi; kp.bj = 32 - bi - bk;
                kp.ilo = (int)fl[0]; kp.klo = (int)fl[2]; kp.jlo = -(1 << (kp.bj - 1));
                // y = 0 sits 256 cells above an aligned block of 512 field values: a frame whose y cells stay within +-256 of the
                // optical axis (1.28 m at the 5 mm leaf) then has constant y bits above the ninth, and the sort of k_crop_runs,
                // which runs on these packed keys, skips the digit they fill (3 passes instead of 4 on the bench frames; with y = 0
                // ON a block boundary every frame straddles it)
                if (kp.bj >= 11) kp.jlo -= 256;
            }
        }
    }
    // Round 4: the single-pass crop also writes the RUNS (one record per run of equal cell key inside a row of 64 input points)
    // and their digit histograms, and the sort runs on the packed cell keys themselves (k_crop_runs, k_voxel.hip)
    bool crop_runs = kp.enabled && c->crop_runs && c->voxel_runs && c->N <= (1 << RUN_SHIFT);
    // 16-byte records x y z rgb (the D435 driver's layout): k_crop_runs leaves the kept points where they are and the centroid
    // kernel reads the input (0.5 GB less written and the same bytes read per 256-frame batch); any other layout is copied
    const bool direct_pts = c->crop_direct && stride == 16 && (rgb_off == 12 || rgb_off < 0) && (reinterpret_cast<uintptr_t>(d_in) & 15u) == 0;
    int st = CD_OK;
    // (the ticket counters reset themselves at the end of every launch that uses them; zeroed here too so that a call that
    // failed half way can never leave the next one with a counter that is not zero)
    ZERO_FILL(c, c->d_ticket, sizeof(int) * (size_t)F * TICKET_PITCH);
    // (kernels write the pinned mirror of the FrameState array themselves where a whole copy launch used to follow them:
    // CUBOID_MIRROR_WRITES=0 restores the copies)
    FrameState* const fs_mirror = c->mirror_writes && c->copy_kernels ? c->h_fs : nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (!(attempt == 0 && c->fs_initialised)) HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState) * F, hipMemcpyHostToDevice));   // (a fused call's zero launch set them)
        c->fs_initialised = false;
        // (the rare redo, and the crops that use d_tileA themselves: from here on every stage fills its own arrays again)
        if (attempt > 0 || !(kp.enabled && crop_runs)) c->batch_zeroed = false;
        ZERO_FILL(c, c->d_tileA, sizeof(int) * (size_t)F * T);
        if (kp.enabled && crop_runs) {
            ZERO_FILL(c, c->d_tile64, sizeof(unsigned long long) * (size_t)F * T);
            ZERO_FILL(c, c->d_ghist, sizeof(uint32_t) * (size_t)F * SORT_MAX_PASSES_HOST * RADIX);
            LAUNCH(c, launch_crop_runs(c->stream, d_in, stride, N, c->N, F, rgb_off, lim, T, p->leaf_size, kp, c->d_fs, c->d_tile64, c->d_cpt, c->d_key[0], c->d_val[0],
                             c->d_ghist, c->d_ticket, direct_pts ? 1 : 0));
            LAUNCH(c, launch_voxel_setup(c->stream, c->d_fs, F, p->leaf_size, c->d_ghist, fs_mirror));
        } else if (kp.enabled) {
            LAUNCH(c, launch_crop_fused(c->stream, d_in, stride, N, c->N, F, rgb_off, lim, T, p->leaf_size, kp, c->d_fs, c->d_tileA, c->d_cpt, c->d_key[0], c->d_ticket));
            LAUNCH(c, launch_voxel_setup(c->stream, c->d_fs, F, p->leaf_size, nullptr, fs_mirror));
        } else {
            LAUNCH(c, launch_crop_count(c->stream, d_in, stride, N, F, rgb_off, lim, T, c->d_fs, c->d_tileA));
            LAUNCH(c, launch_scan_tiles(c->stream, c->d_tileA, F, T, FS_FIELD(c, n_c), FS_PITCH));
            LAUNCH(c, launch_voxel_setup(c->stream, c->d_fs, F, p->leaf_size, nullptr, fs_mirror));
            LAUNCH(c, launch_crop_compact(c->stream, d_in, stride, N, c->N, F, rgb_off, lim, T, p->leaf_size, c->d_fs, c->d_tileA, c->d_cpt, c->d_key[0]));
        }
        st = sync_fs(c, F, fs_mirror != nullptr);   // sync #1: n_c, key_bits (sort pass count); the mirror was written by k_voxel_setup
        if (st) return st;
        bool over = false;
        for (int f = 0; f < F; ++f) over = over || c->h_fs[f].crop_overflow != 0;
        if (!over) break;
        if (std::getenv("CUBOID_DEBUG")) std::fprintf(stderr, "cuboid_hip: single-pass crop overflowed, redoing the batch in two passes\n");
        kp.enabled = 0;       // rare: redo the crop in two passes (the FrameState init in h_fs was overwritten by the sync)
        crop_runs = false;
        for (int f = 0; f < F; ++f) {
            FrameState& s = c->h_fs[f];
            std::memset(&s, 0, sizeof(s));
            for (int a = 0; a < 3; ++a) { s.mn[a] = 0xffffffffu; s.mx[a] = 0u; }
            }
    }
    int max_nc = 0, max_bits = 0;
    for (int f = 0; f < F; ++f) { max_nc = std::max(max_nc, c->h_fs[f].n_c); max_bits = std::max(max_bits, c->h_fs[f].key_bits); }
    const int Tc = std::max(1, (max_nc + TILE - 1) / TILE);
    const int Tsc = std::max(1, (max_nc + SORT_TILE - 1) / SORT_TILE);          // tiles of k_voxel_runs / k_radix_ghist
    const int Tscat = std::max(1, (max_nc + SCATTER_TILE - 1) / SCATTER_TILE);   // tiles of the scatters (their own size: common.hpp)
    const int npass = (max_bits + RADIX_BITS - 1) / RADIX_BITS;
    int cur = 0;
    // By runs (default): the sort moves one element per run of equal voxel index among the cropped points - they are in image
    // order, 2.4 points per run on the bench frames - and the centroid kernel reads the runs' points contiguously; the bound
    // on the tiles is the point count (the run count is only known on the device).  CUBOID_VOXEL_RUNS=0: sort the points.
    const bool by_runs = c->voxel_runs && npass > 0 && c->N <= (1 << RUN_SHIFT);   // (a run's start takes RUN_SHIFT bits of its payload)
    int Tc_runs = Tc;
    uint32_t* const key[2] = {c->d_key[0], c->d_key[1]}, * const val[2] = {c->d_val[0], c->d_val[1]};
    if (crop_runs) {
        // the runs and their histograms are there already; which of the packed key's four digits vary in some frame?
        int vary = 0, max_runs = 0;
        for (int f = 0; f < F; ++f) {
            if (c->h_fs[f].n_c > 0) vary |= c->h_fs[f].digit_vary;
            max_runs = std::max(max_runs, c->h_fs[f].n_runs);
        }
        int digits[4], nd = 0;
        for (int d = 0; d < 4; ++d) if ((vary >> d) & 1) digits[nd++] = d;
        const int Tsr = std::max(1, (max_runs + SCATTER_TILE - 1) / SCATTER_TILE);   // (the run count is known here: tighter than the point count)
        Tc_runs = std::max(1, (max_runs + TILE - 1) / TILE);
        LAUNCH(c, cur = launch_radix_scatter_runs(c->stream, key, val, c->N, F, Tsr, digits, nd, c->d_fs, c->d_ghist, c->d_sstate, c->d_ticket));
    } else if (by_runs)
        LAUNCH(c, cur = launch_radix_sort_runs(c->stream, key, val, c->N, F, T, Tsc, Tscat, npass, c->d_fs, c->d_ghist, c->d_sstate, c->d_tileA, kp, c->d_ticket));
    else
        LAUNCH(c, cur = launch_radix_sort(c->stream, key, val, c->N, F, Tsc, Tscat, npass, c->d_fs, c->d_ghist, c->d_sstate, kp, c->d_ticket));
    if (cur < 0) return fail(c, CD_ERR_DEVICE, "radix sort: the scan state could not be zeroed");
    const uint32_t* vin = c->d_val[cur];   // zero passes (empty frames only): the permutation is never read
    // voxel heads + centroids in one kernel: n_v (0 from the FrameState init for empty frames) and every tile's output
    // offset come from a chained scan (state in d_tileA)
    ZERO_FILL(c, c->d_tileC, sizeof(int) * (size_t)F * T);
    if (crop_runs || by_runs)
        LAUNCH(c, launch_voxel_centroid_runs(c->stream, c->d_key[cur], vin, crop_runs && direct_pts ? reinterpret_cast<const float4*>(d_in) : c->d_cpt, c->N, F, T, crop_runs ? Tc_runs : Tc,
                                             rgb_off >= 0 ? 1 : 0, c->d_fs, c->d_tileC, c->d_vox, c->d_ticket, c->centroid_lanes, crop_runs && direct_pts ? N : c->N));
    else
        LAUNCH(c, launch_voxel_centroid(c->stream, c->d_key[cur], vin, c->d_cpt, c->N, F, T, Tc, rgb_off >= 0 ? 1 : 0, c->d_fs, c->d_tileC, c->d_vox, c->d_ticket));
    if (rounds_out) *rounds_out = 0;
    return CD_OK;
}

// S2.  in: d_vox + fs.n_v (host mirror h_fs[].n_v must be current).  out: h_model/h_have refined,
// fs.status updated for NO_MODEL, iterations per frame.
// axes: per-frame constraint axes of a constrained model, 3 floats per frame (nullptr: p->plane_axis for every frame)
int stage_plane(cd_context* c, int F, const cd_params* p, std::vector<int>& iterations, int* rounds_out, const float* axes = nullptr) {
    const int T = c->T;
    const bool mr = c->mirror_reads != 0;
    const float thr = hm::fold_ge(p->plane_distance_threshold);
    int max_nv = 0;
    for (int f = 0; f < F; ++f) max_nv = std::max(max_nv, c->h_fs[f].n_v);
    const int Tv = std::max(1, (max_nv + TILE - 1) / TILE);
    std::vector<hm::RansacReplay> rep(F);
    iterations.assign(F, 0);
    for (int f = 0; f < F; ++f) c->h_active[f] = (c->h_fs[f].status == CD_OK || c->h_fs[f].status == CD_ERR_NO_MODEL) ? 1 : 0;
    ZERO_FILL(c, c->d_counts, sizeof(int) * (size_t)F * MAX_HYP);
    const int targets[4] = {16, 64, 256, MAX_HYP};
    const int h_cap = std::min(MAX_HYP, p->plane_max_iterations + 40);   // max_iterations+1 plus 39 skipped models
    int h_prev = 0, rounds = 0;
    for (int r = 0; r < 4; ++r) {
        const int h_target = std::min(targets[r], h_cap);
        if (h_target <= h_prev) break;
        // (mirror reads: the kernels read the few per-frame words the host decides - active flags, chosen models - straight from
        // the pinned host arrays, which the device sees; CUBOID_MIRROR_READS=0 uploads them first as rounds 1-5 did)
        if (!mr) HIPCHK(c, xfer(c, c->d_active, c->h_active, sizeof(int) * F, hipMemcpyHostToDevice));
        const int* active_p = mr ? c->h_active : c->d_active;
        LAUNCH(c, launch_ransac_sample(c->stream, c->d_vox, c->N, F, c->d_fs, c->d_rnd, h_target, active_p, c->d_models, c->d_valid));
        LAUNCH(c, launch_ransac_count(c->stream, c->d_vox, c->N, F, Tv, c->d_fs, c->d_models, c->d_valid, active_p, h_prev, h_target, thr, c->d_counts));
        // only the first h_target columns of the [F][MAX_HYP] tables are live: one strided copy each
        {   // (one launch: the three tables and - sync_fs below finds it done - nothing else; the FrameState read-back follows)
            XferBatch xb(c);
            xb.add2d(c->h_counts, sizeof(int) * MAX_HYP, c->d_counts, sizeof(int) * MAX_HYP, sizeof(int) * h_target, F, hipMemcpyDeviceToHost);
            xb.add2d(c->h_valid, sizeof(int) * MAX_HYP, c->d_valid, sizeof(int) * MAX_HYP, sizeof(int) * h_target, F, hipMemcpyDeviceToHost);
            xb.add2d(c->h_models, sizeof(float4) * MAX_HYP, c->d_models, sizeof(float4) * MAX_HYP, sizeof(float4) * h_target, F, hipMemcpyDeviceToHost);
            xb.add(c->h_fs, c->d_fs, sizeof(FrameState) * F, hipMemcpyDeviceToHost);
            HIPCHK(c, xb.flush());
        }
        int st = sync_fs(c, F, /*copied=*/true);   // sync #2 (per round): counts + n_hyp
        if (st) return st;
        ++rounds;
        bool all_done = true;
        for (int f = 0; f < F; ++f) {
            if (!c->h_active[f]) continue;
            const FrameState& s = c->h_fs[f];
            if (p->plane_model != CD_PLANE) {   // constrained models: a hypothesis off the axis constraint scores 0 inliers
                for (int h = rep[f].pos; h < s.n_hyp; ++h) {
                    const float4 m = c->h_models[(size_t)f * MAX_HYP + h];
                    const float mm[4] = {m.x, m.y, m.z, m.w};
                    if (c->h_valid[(size_t)f * MAX_HYP + h] && !hm::plane_model_valid(p->plane_model, mm, axes ? axes + 3 * f : p->plane_axis, p->plane_eps_angle))
                        c->h_counts[(size_t)f * MAX_HYP + h] = 0;
                }
            }
            const bool fin = rep[f].consume(c->h_counts + (size_t)f * MAX_HYP, c->h_valid + (size_t)f * MAX_HYP, s.n_hyp, std::max(1, s.n_v),
                                            p->plane_max_iterations, p->plane_probability, s.sampler_exhausted != 0 || h_target >= h_cap);
            if (fin) c->h_active[f] = 0; else all_done = false;
        }
        h_prev = h_target;
        if (all_done) break;
    }
    if (rounds_out) *rounds_out = rounds;
    // chosen models -> device; moments of their inliers -> host eigen33 -> refined models
    for (int f = 0; f < F; ++f) {
        iterations[f] = rep[f].iterations;
        c->h_have[f] = rep[f].best_h >= 0 ? 1 : 0;
        c->h_model[f] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c->h_have[f]) c->h_model[f] = c->h_models[(size_t)f * MAX_HYP + rep[f].best_h];
    }
    // selectWithinDistance of a constrained model returns nothing when the model violates the constraint: the
    // device then sees "no model" (h_active doubles as the pinned staging copy), the host keeps reporting it
    auto upload_have = [&](const float4* models_too = nullptr) -> int {
        for (int f = 0; f < F; ++f) {
            const float mm[4] = {c->h_model[f].x, c->h_model[f].y, c->h_model[f].z, c->h_model[f].w};
            c->h_active[f] = c->h_have[f] && hm::plane_model_valid(p->plane_model, mm, axes ? axes + 3 * f : p->plane_axis, p->plane_eps_angle) ? 1 : 0;
        }
        if (mr) return CD_OK;   // (the kernels read h_model / h_active)
        XferBatch xb(c);
        if (models_too) xb.add(c->d_model, models_too, sizeof(float4) * F, hipMemcpyHostToDevice);
        xb.add(c->d_have, c->h_active, sizeof(int) * F, hipMemcpyHostToDevice);
        HIPCHK(c, xb.flush());
        return CD_OK;
    };
    if (int st = upload_have(&c->h_model[0])) return st;   // (the chosen models ride along: one launch)
    if (p->plane_optimize) {
        ZERO_FILL(c, c->d_sums, sizeof(unsigned long long) * 10 * F);
        LAUNCH(c, launch_plane_cov(c->stream, c->d_vox, c->N, F, Tv, c->d_fs, mr ? c->h_model : c->d_model, mr ? c->h_active : c->d_have, thr, c->d_sums));
        HIPCHK(c, xfer(c, c->h_sums, c->d_sums, sizeof(unsigned long long) * 10 * F, hipMemcpyDeviceToHost));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // sync #3
        for (int f = 0; f < F; ++f) {
            if (!c->h_have[f]) continue;
            float in[4] = {c->h_model[f].x, c->h_model[f].y, c->h_model[f].z, c->h_model[f].w}, out[4];
            hm::plane_refit_from_moments((const uint64_t*)(c->h_sums + 10 * (size_t)f), in, out);
            c->h_model[f] = make_float4(out[0], out[1], out[2], out[3]);
        }
        if (!mr) HIPCHK(c, xfer(c, c->d_model, c->h_model, sizeof(float4) * F, hipMemcpyHostToDevice));
        if (p->plane_model != CD_PLANE) {
            HIPCHK(c, hipStreamSynchronize(c->stream));   // h_active is about to be rewritten
            if (int st = upload_have()) return st;
        }
    }
    (void)T;
    return CD_OK;
}

// S3 (+S3b).  out: d_plane_idx, d_obj, fs.n_plane, fs.n_o
int stage_extract(cd_context* c, int F, const cd_params* p, int gate_mode = -1) {
    const int T = c->T;
    const float thr = hm::fold_ge(p->plane_distance_threshold);
    int max_nv = 0;
    for (int f = 0; f < F; ++f) max_nv = std::max(max_nv, c->h_fs[f].n_v);
    const int Tv = std::max(1, (max_nv + TILE - 1) / TILE);
    const float z2lo = hm::fold_ge(p->crop2_z_min), z2hi = hm::fold_le(p->crop2_z_max);
    BBoxGate gate;
    std::memset(&gate, 0, sizeof(gate));
    gate.enable = gate_mode >= 0 ? gate_mode : (p->bbox_enable ? 1 : 0);
    for (int i = 0; i < 12; ++i) gate.P[i] = p->bbox_P[i];
    for (int i = 0; i < 4; ++i) gate.rect[i] = (float)p->bbox_rect[i];
    const float4* model_p = c->mirror_reads ? c->h_model : c->d_model;   // (see stage_plane)
    const int* have_p = c->mirror_reads ? c->h_active : c->d_have;
    ZERO_FILL(c, c->d_tileA, sizeof(int) * (size_t)F * T);
    ZERO_FILL(c, c->d_tileB, sizeof(int) * (size_t)F * T);
    LAUNCH(c, launch_plane_flag_count(c->stream, c->d_vox, c->N, F, T, Tv, c->d_fs, model_p, have_p, thr, p->extract_negative, p->crop2_enable, z2lo, z2hi, gate, c->call_rects, c->d_tileA, c->d_tileB));
    {   // both scans in one launch; the two totals also go straight into the host's FrameState mirror (nothing else of it changes here)
        const bool mirrored = c->mirror_writes && c->copy_kernels;
        const ScanJob ja{c->d_tileA, FS_FIELD(c, n_plane), mirrored ? (int*)((char*)c->h_fs.get() + offsetof(FrameState, n_plane)) : nullptr};
        const ScanJob jb{c->d_tileB, FS_FIELD(c, n_o), mirrored ? (int*)((char*)c->h_fs.get() + offsetof(FrameState, n_o)) : nullptr};
        LAUNCH(c, launch_scan_tiles2(c->stream, ja, jb, F, T, FS_PITCH));
    }
    LAUNCH(c, launch_extract_scatter(c->stream, c->d_vox, c->N, F, T, Tv, c->d_fs, model_p, have_p, thr, p->extract_negative, p->crop2_enable, z2lo, z2hi, gate, c->call_rects, c->d_tileA, c->d_tileB, c->d_plane_idx, c->d_obj));
    return CD_OK;
}

// S5.  in: d_obj + fs.n_o (device).  out: d_label, d_sizes, fs.n_k/ksize/koff, d_src0/d_src
int stage_cluster(cd_context* c, int F, const cd_params* p, int max_no_hint, bool force_global = false) {
    const int T = c->T;
    const int To = std::max(1, (max_no_hint + TILE - 1) / TILE);
    const float cell = (float)(p->cluster_tolerance * (1.0 + 1.0 / 1024.0));
    const float inv_cell = 1.0f / cell;
    const float r2 = (float)(p->cluster_tolerance * p->cluster_tolerance);
    if (p->cluster_enable) {
        // frames with <= 8192 object points (the usual case) are clustered by one workgroup in LDS, over cells small
        // enough (edge just under tol / sqrt(3)) that the points of one cell are connected by construction ...
        const float small_cell = (float)(p->cluster_tolerance / std::sqrt(3.0) * (1.0 - 1.0 / 1024.0));
        LAUNCH(c, launch_cluster_lds(c->stream, c->d_obj, c->N, F, c->d_fs, 1.0f / small_cell, r2, c->d_parent, c->d_csize, c->d_rank));
    }
    const bool by_cells = c->cluster_cells && !force_global;
    if (p->cluster_enable && max_no_hint > 8192 && by_cells) {
        // ... larger ones by the same cell graph with the points in global memory (k_cluster_cells; d_src is free until the labels
        // are scattered) ...
        const float small_cell = (float)(p->cluster_tolerance / std::sqrt(3.0) * (1.0 - 1.0 / 1024.0));
        LAUNCH(c, launch_cluster_cells(c->stream, c->d_obj, c->N, F, c->d_fs, 1.0f / small_cell, r2, c->d_parent, c->d_csize, c->d_rank, c->d_src));
    }
    if (p->cluster_enable && ((max_no_hint > 8192 && !by_cells) || force_global)) {
        // ... and the rare frame whose cells do not fit the table (fs.cl_done == 0) by the point-graph kernels in global memory
        HIPCHK(c, hipMemsetAsync(c->d_head, 0xff, sizeof(int) * (size_t)F * CELL_BUCKETS, c->stream));
        LAUNCH(c, launch_cluster_build(c->stream, c->d_obj, c->N, F, To, c->d_fs, inv_cell, c->d_head, c->d_next, c->d_parent, c->d_csize, c->d_rank));
        LAUNCH(c, launch_cluster_hook(c->stream, c->d_obj, c->N, F, To, c->d_fs, inv_cell, r2, c->d_head, c->d_next, c->d_parent));
        LAUNCH(c, launch_cluster_flatten(c->stream, c->N, F, To, c->d_fs, c->d_parent, c->d_csize));
    }
    LAUNCH(c, launch_cluster_rank(c->stream, c->N, F, c->d_fs, p->cluster_enable, p->cluster_min_size, p->cluster_max_size, c->d_parent, c->d_csize, c->d_cand, c->d_rank, c->d_sizes, c->mirror_writes && c->copy_kernels ? c->h_fs : nullptr));
    ZERO_FILL(c, c->d_tileK, sizeof(int) * (size_t)F * KICP * T);
    LAUNCH(c, launch_label_count(c->stream, c->N, F, T, To, c->d_fs, p->cluster_enable, c->d_parent, c->d_rank, c->d_label, c->d_tileK, 0));
    LAUNCH(c, launch_scan_tiles(c->stream, c->d_tileK, F * KICP, T, nullptr, 0));
    LAUNCH(c, launch_label_scatter(c->stream, c->d_obj, c->N, F, T, To, c->d_fs, c->d_label, c->d_tileK, c->d_src0, c->d_src, 0, nullptr));
    return CD_OK;
}

// stage_cluster + sync; when the LDS kernel gave a frame up (too many cells / too wide a cloud for its table) and the
// global-memory kernels were not part of the launch, the stage is run again with them.
int stage_cluster_sync(cd_context* c, int F, const cd_params* p, int max_no) {
    const bool mirrored = c->mirror_writes && c->copy_kernels;   // (k_cluster_rank wrote the FrameState mirror)
    int st = stage_cluster(c, F, p, max_no);
    if (st) return st;
    st = sync_fs(c, F, mirrored);
    if (st || !p->cluster_enable || (max_no > 8192 && !c->cluster_cells)) return st;   // (the point-graph kernels were part of the launch)
    bool left = false;
    for (int f = 0; f < F; ++f) left = left || (c->h_fs[f].n_o > 0 && !c->h_fs[f].cl_done);
    if (!left) return CD_OK;
    if (std::getenv("CUBOID_DEBUG")) std::fprintf(stderr, "cuboid_hip: LDS clustering gave frames up, running the global-memory path\n");
    c->batch_zeroed = false;   // (d_tileK has been used: the redo fills it again)
    st = stage_cluster(c, F, p, max_no, true);
    if (st) return st;
    return sync_fs(c, F, mirrored);
}

// IcpCluster records h_cl[first .. first + n) of the clusters 0 .. n-1 of one frame against template `slot`: sizes size[0..n),
// sources at base + off[0..n) in d_src0 / d_src
void set_icp_clusters(cd_context* c, int first, int n, int frame, const int* size, const int* off, int base, int slot) {
    for (int k = 0; k < n; ++k) c->h_cl[first + k] = IcpCluster{base + off[k], size[k], frame, k, c->tpl_off[slot], c->tpl_m[slot], 0, slot};
}

// ---- S6: ICP ------------------------------------------------------------------------------------------------------------------
// stage_icp plans the stage on the host (plan_icp), issues what every driver needs (icp_setup), then hands the clusters to the
// drivers in turn: k_icp_lat for lattice templates, the grouped k_icp_pipe launches for several templates, the whole-cluster
// launch, the persistent launch for a few clusters, and the sliced multi-launch loop for whatever is left.  A driver sets
// *done when it has run the stage to its end (records read back, stream synchronised); otherwise the drivers after it take
// the clusters it left and find the ones it ran finished in d_st / h_st (the stream orders them).

// kind: 0 = no persistent kernel can take the template, 1 = k_icp_pipe (LDS-resident, gridded), 2 = k_icp_pipe_big (global memory)
int tpl_kind(const cd_context* c, const IcpCluster& cl) {
    if (cl.tpl_m <= 0 || !c->tpl_gridded[cl.slot]) return 0;
    if (cl.tpl_m <= ICP_TPL_LDS) return 1;
    return c->tpl_big[cl.slot] ? 2 : 0;
}

struct TplGroup { int beg, end, live; int kind; long long pts; };

struct IcpPlan {   // host-side decisions of one ICP stage (plan_icp)
    int ncl = 0, guess_mode = CD_GUESS_NONE, max_n = 0, qslice = 0;
    size_t guess_need = 0;                       // floats of the guess upload
    const std::vector<float>* frame_guess = nullptr;   // per-frame guesses: cd_set_frame_guesses' or (CD_GUESS_SURFACE) the call's own
    std::vector<char> in_lat;                    // the cluster takes k_icp_lat
    int n_lat = 0, n_live = 0, lat_max_n = 0;
    std::vector<TplGroup> groups;
    int nwork = 0;                               // items of the sliced work list (h_work)
    int wg_cap = 0;                              // workgroups of a persistent ICP launch at most (CUBOID_ICP_MAX_WG)
    bool grouped_pipe = false, lat_direct = false, pipe_ok = false, big_ok = false, whole_cluster = false;
    bool pre_zeroed = false;                     // (icp_setup) d_acc / d_accf / d_queue were zeroed by the fused call
    bool crowded = false;                        // (icp_params) four or more batches in flight on the device
};

// Clusters h_cl[0..ncl) -> plan; fills the work list h_work, tile0 of every cluster and the initial states h_st.
int plan_icp(cd_context* c, int ncl, const cd_params* p, IcpPlan* pl) {
    pl->ncl = ncl;
    // initial guess (pcl::Registration::align(output, guess)); the default - and the reference's live path - is none
    // (CD_GUESS_SURFACE is CD_GUESS_PER_FRAME with the guesses the call derived itself)
    const int guess_mode = pl->guess_mode = p->icp_use_guess == CD_GUESS_SURFACE ? CD_GUESS_PER_FRAME : p->icp_use_guess;
    pl->frame_guess = p->icp_use_guess == CD_GUESS_SURFACE ? &c->surface_guess : &c->frame_guess;
    if (guess_mode != CD_GUESS_NONE) {
        int max_frame = 0;
        for (int k = 0; k < ncl; ++k) { pl->max_n = std::max(pl->max_n, c->h_cl[k].n); max_frame = std::max(max_frame, c->h_cl[k].frame); }
        pl->guess_need = guess_mode == CD_GUESS_PER_FRAME ? 16 * ((size_t)max_frame + 1) : (guess_mode == CD_GUESS_CLUSTER ? 16 * (size_t)ncl : 16);
        if (guess_mode == CD_GUESS_PER_FRAME && pl->frame_guess->size() < pl->guess_need) return fail(c, CD_ERR_INVALID_ARG, "icp_use_guess = CD_GUESS_PER_FRAME but cd_set_frame_guesses holds fewer frames than the batch");
    }
    // queries per workgroup: 512 when the batch fills the chip, smaller slices (more workgroups) otherwise
    long long qtot = 0;
    for (int k = 0; k < ncl; ++k) qtot += c->h_cl[k].n;
    pl->qslice = std::max(64, std::min(ICP_QSLICE, (int)((qtot / 512 + 15) / 16 * 16)));
    // Template groups: runs of clusters that share a template (one run per template when every cluster is matched against
    // every template).  With several templates in the batch, the groups whose template is LDS-resident and gridded go through
    // ONE k_icp_pipe launch (each group gets a share of the workgroups and its own queue) when there are enough of them to
    // fill a fifth of the chip; the other clusters take the sliced driver.
    // Clusters whose template is a lattice (every make_cuboid.py template; IcpLattice, common.hpp) go to k_icp_lat - closed-form
    // nearest neighbour, one workgroup per cluster - and take no part in the grouping.  CUBOID_ICP_LATTICE=0 and the
    // forced driver modes (CUBOID_ICP_MODE) keep them on the generic searches (A/B, and the GPU suite runs under each mode).
    const bool use_lat = c->icp_lattice != 0 && c->icp_mode == 0;
    pl->in_lat.assign((size_t)ncl, 0);
    for (int k = 0; k < ncl; ++k) {
        const IcpCluster& cl = c->h_cl[k];
        const bool live = cl.n >= 3 && cl.tpl_m > 0;
        pl->n_live += live ? 1 : 0;
        if (use_lat && live && c->tpl_faces[cl.slot] > 0) { pl->in_lat[(size_t)k] = 1; ++pl->n_lat; pl->lat_max_n = std::max(pl->lat_max_n, cl.n); }
    }
    c->timing.icp_search = pl->n_lat == 0 ? 0 : (pl->n_lat == pl->n_live ? 1 : 2);
    std::vector<TplGroup>& groups = pl->groups;
    for (int k = 0; k < ncl; ++k) {
        const IcpCluster& cl = c->h_cl[k];
        if (groups.empty() || c->h_cl[groups.back().beg].tpl_off != cl.tpl_off || c->h_cl[groups.back().beg].tpl_m != cl.tpl_m)
            groups.push_back(TplGroup{k, k, 0, use_lat && c->tpl_faces[cl.slot] > 0 ? 0 : tpl_kind(c, cl), 0});
        TplGroup& g = groups.back();
        g.end = k + 1;
        if (cl.n >= 3) { g.live += 1; g.pts += cl.n; }
    }
    int n_grouped = 0;
    for (const TplGroup& g : groups) if (g.kind) n_grouped += g.live;
    pl->grouped_pipe = groups.size() > 1 && groups.size() <= 16 && n_grouped > 0 &&
                       (c->icp_mode == 3 || (c->icp_mode == 0 && n_grouped * 5 >= c->n_cu));
    if (std::getenv("CUBOID_DEBUG")) {
        std::fprintf(stderr, "cuboid_hip: stage_icp %d clusters, %zu template groups, %d in pipe groups, grouped_pipe %d:", ncl, groups.size(), n_grouped, (int)pl->grouped_pipe);
        for (const TplGroup& g : groups) std::fprintf(stderr, " [%d,%d) m=%d kind=%d live=%d", g.beg, g.end, c->h_cl[g.beg].tpl_m, g.kind, g.live);
        std::fprintf(stderr, "\n");
    }
    std::vector<char> in_pipe((size_t)ncl, 0);
    if (pl->grouped_pipe)
        for (const TplGroup& g : groups) if (g.kind) for (int k = g.beg; k < g.end; ++k) in_pipe[(size_t)k] = 1;
    int nwork = 0;
    for (int k = 0; k < ncl; ++k) {
        IcpCluster& cl = c->h_cl[k];
        cl.tile0 = nwork;
        const int tiles = cl.n >= 3 && cl.tpl_m > 0 && !in_pipe[(size_t)k] && !pl->in_lat[(size_t)k] ? (cl.n + pl->qslice - 1) / pl->qslice : 0;
        if (nwork + tiles > c->work_cap) return fail(c, CD_ERR_CAPACITY, "ICP work list overflow");
        for (int t = 0; t < tiles; ++t) c->h_work[nwork++] = IcpWork{k, t};
        for (int s = 0; s < 2; ++s) {
            IcpState& st = c->h_st[2 * k + s];
            std::memset(&st, 0, sizeof(st));
            for (int i = 0; i < 4; ++i) st.Tfinal[5 * i] = 1.f;
            if (guess_mode != CD_GUESS_NONE && guess_mode != CD_GUESS_CLUSTER)   // final_transformation_ = guess (CD_GUESS_CLUSTER: k_shape_frames writes it on the device)
                std::memcpy(st.Tfinal, guess_mode == CD_GUESS_PER_FRAME ? pl->frame_guess->data() + 16 * (size_t)cl.frame : p->icp_guess, 64);
            st.prev_mse = std::numeric_limits<double>::max();
            if (cl.tpl_m <= 0) { st.done = 1; st.status = CD_ERR_NO_TEMPLATE; }
            else if (cl.n < 3) { st.done = 1; st.status = CD_ERR_FEW_CORRESPONDENCES; }
        }
    }
    pl->nwork = nwork;
    pl->wg_cap = c->icp_max_wg > 0 ? std::min(c->icp_max_wg, c->n_cu) : c->n_cu;
    // A stage whose clusters ALL take k_icp_lat (the default template, no initial guess): the kernel reads the cluster list, the
    // order and the initial states from the pinned host arrays and writes the final states and fitness sums there - a few
    // hundred bytes per cluster once at each end of its ICP - instead of three copy launches around it.
    pl->lat_direct = c->icp_direct && pl->n_lat > 0 && pl->n_lat == pl->n_live && guess_mode == CD_GUESS_NONE && c->mirror_reads && c->mirror_writes && c->copy_kernels;
    // Batch mode: with at least ~n_cu/5 clusters every CU can own whole clusters, so each cluster runs its
    // complete ICP (all iterations + fitness) inside one persistent workgroup, one launch for the batch.
    // The pipelined variant (two to four clusters in flight per workgroup, no barrier in the iteration loop) needs one
    // LDS-resident gridded template shared by every cluster of the launch; otherwise k_icp_cluster runs.
    bool one_tpl = true;
    for (int k = 1; k < ncl && one_tpl; ++k) one_tpl = c->h_cl[k].tpl_off == c->h_cl[0].tpl_off && c->h_cl[k].tpl_m == c->h_cl[0].tpl_m;
    pl->pipe_ok = c->icp_mode != 2 && one_tpl && tpl_kind(c, c->h_cl[0]) == 1;
    // ... or, for a template that does not fit LDS, its twin that reads the template from global memory (k_icp_pipe_big)
    pl->big_ok = c->icp_mode != 2 && one_tpl && tpl_kind(c, c->h_cl[0]) == 2;
    // (auto mode: only the pipelined kernel beats the sliced driver; with mixed or non-resident templates k_icp_cluster's
    // barrier per iteration costs more than it saves, so those batches stay sliced unless the mode is forced)
    // (measured crossover on the bench frames: 33 clusters 3.3 ms sliced / 3.7 ms pipelined, 65 clusters 4.4 / 3.9, 130 clusters
    // 6.4 / 4.0: the pipelined kernel wins from about a fifth of the CUs' worth of clusters)
    pl->whole_cluster = !pl->grouped_pipe && (c->icp_mode >= 2 || (c->icp_mode == 0 && ncl * 5 >= c->n_cu && (pl->pipe_ok || pl->big_ok)));
    return CD_OK;
}

// which guess k_icp_apply_guess moves problem k by: the only one, its frame's, its own
int guess_indexing(int guess_mode) { return guess_mode == CD_GUESS_PER_FRAME ? 1 : (guess_mode == CD_GUESS_CLUSTER ? 2 : 0); }

// the record of a slot's template as the device table holds it: an empty slot can give no guess
ShapeFrame template_frame(const cd_context* c, int slot) {
    if (slot >= 0 && slot < CD_MAX_TEMPLATES && c->tpl_m[slot] > 0) return c->tpl_frame[slot];
    ShapeFrame none;
    shape_empty(0, CD_ERR_NO_TEMPLATE, &none);
    return none;
}

// CD_GUESS_CLUSTER: k_shape_frames over the stage's ncl problems (d_cl, d_src0) -> d_shape, d_guess and Tfinal of d_st.  The
// template table goes up first when a template has changed since the last time (a copy launch from its pinned mirror: no
// synchronisation).  The buffers have been sized by icp_setup.
int launch_cluster_guesses(cd_context* c, int ncl) {
    if (c->tframe_dirty) {
        for (int s = 0; s < CD_MAX_TEMPLATES; ++s) c->h_tframe[s] = template_frame(c, s);
        HIPCHK(c, xfer(c, c->d_tframe, c->h_tframe, sizeof(ShapeFrame) * CD_MAX_TEMPLATES, hipMemcpyHostToDevice));
        c->tframe_dirty = false;
    }
    LAUNCH(c, launch_shape_frames(c->stream, ncl, c->d_cl, c->d_src0, c->d_shape, c->d_tframe, c->d_guess, c->d_st));
    return CD_OK;
}

// the stream operations every driver needs before the stage's start event: guess, cluster list, work list, initial states,
// zeroed sums, guess applied to the sources
int icp_setup(cd_context* c, const cd_params* p, IcpPlan* pl) {
    const int ncl = pl->ncl;
    if (pl->guess_mode != CD_GUESS_NONE) {
        GROW(c, d_guess, pl->guess_need);
        if (pl->guess_mode == CD_GUESS_CLUSTER) {   // (the guesses are written on the device; the records' buffers before anything is on the stream)
            GROW(c, d_shape, (size_t)ncl); GROW(c, h_shape, (size_t)ncl);
            GROW(c, d_tframe, (size_t)CD_MAX_TEMPLATES); GROW(c, h_tframe, (size_t)CD_MAX_TEMPLATES);
        } else
            HIPCHK(c, copy_sync(c, c->d_guess, pl->guess_mode == CD_GUESS_PER_FRAME ? pl->frame_guess->data() : p->icp_guess, sizeof(float) * pl->guess_need, hipMemcpyHostToDevice));
    }
    if (!pl->lat_direct) {
        XferBatch xb(c);   // (one launch)
        xb.add(c->d_cl, c->h_cl, sizeof(IcpCluster) * ncl, hipMemcpyHostToDevice);
        if (pl->nwork > 0) xb.add(c->d_work, c->h_work, sizeof(IcpWork) * pl->nwork, hipMemcpyHostToDevice);
        xb.add(c->d_st, c->h_st, sizeof(IcpState) * 2 * ncl, hipMemcpyHostToDevice);
        HIPCHK(c, xb.flush());
    }
    // (zeroed up front by the fused call for its FIRST ICP stage only: a batch that runs one stage per template fills them again)
    pl->pre_zeroed = c->batch_zeroed;
    c->batch_zeroed = false;
    if (!pl->pre_zeroed) {
        HIPCHK(c, hipMemsetAsync(c->d_acc, 0, sizeof(unsigned long long) * 48 * (size_t)ncl, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_accf, 0, sizeof(unsigned long long) * ((size_t)ncl + 1), c->stream));   // (+ the wave-time word of k_icp_lat)
    }
    if (c->icp_bounded) {   // rule C8: the sliced / persistent drivers' correspondence counts, [cluster][it % 3]
        GROW(c, d_ncorr, 3 * (size_t)ncl);
        HIPCHK(c, hipMemsetAsync(c->d_ncorr, 0, sizeof(uint32_t) * 3 * (size_t)ncl, c->stream));
    }
    if (pl->guess_mode == CD_GUESS_CLUSTER) {   // rule C13: record, guess and Tfinal of every problem, after the d_cl / d_st upload above
        if (int e = launch_cluster_guesses(c, ncl)) return e;
        HIPCHK(c, xfer(c, c->h_shape, c->d_shape, sizeof(ShapeFrame) * (size_t)ncl, hipMemcpyDeviceToHost));   // (on the host by the stage's final synchronisation)
    }
    if (pl->guess_mode != CD_GUESS_NONE)   // input_transformed = guess * source (d_src is a copy of d_src0 at this point)
        LAUNCH(c, launch_icp_apply_guess(c->stream, ncl, pl->max_n, c->d_cl, c->d_guess, guess_indexing(pl->guess_mode), c->d_src0, c->d_src));
    return CD_OK;
}

IcpParams icp_params(const cd_context* c, const cd_params* p, bool* crowded) {
    IcpParams ip;
    ip.max_iter = p->icp_max_iterations;
    ip.grid_rc = 1.0f;
    if (const char* e = std::getenv("CUBOID_ICP_GRID_RC")) ip.grid_rc = (float)std::atof(e);
    ip.trans_eps = p->icp_transformation_epsilon;
    ip.rel_mse = p->icp_euclidean_fitness_epsilon;
    ip.rot_thr = 1.0 - p->icp_transformation_epsilon;
    ip.abs_mse = 1e-12;
    // Whole-cluster launches: how many clusters a workgroup keeps in flight and how many workgroups there are.  A call that has
    // the device to itself wants every CU at work: one workgroup per CU (or per cluster), two slots, the second filled as long
    // as clusters are left.  With other calls in flight (BatchPipeline) the chip is full anyway and what counts is the CU-time
    // a batch costs: FOUR clusters per workgroup keep its sixteen waves supplied while one of them solves a step (no wave waits
    // at a hand-over, no workgroup ends with one cluster alone), on a quarter as many workgroups - the other batches have the
    // other CUs (config 3, 522 clusters: 2 x 256 -> 4 x 128 is 48.4 -> 53.3 k frames/s; grids that are not a multiple of 32 -
    // 4 per XCD and shader engine - lose 2-4 %).
    // (crossover measured on config 3: with two calls in flight the two shapes tie, with three 2 x 256 wins 49.4 : 46.5 k, with
    // four 4 x 128 wins 52.9 : 49.7 k - and the last launches of a burst, which soon have the GPU to themselves, spread out)
    *crowded = g_batches_in_flight[c->device & (MAX_DEVICES - 1)].load() >= 4;
    ip.pipe_slots = c->icp_slots > 0 ? std::min(c->icp_slots, CD_PIPE_SLOTS) : (*crowded ? CD_PIPE_SLOTS : std::min(2, CD_PIPE_SLOTS));
    ip.donate = 0;   // (set by icp_run_whole for a launch that has the GPU to itself)
    ip.don = c->d_don;
    ip.don_idle = c->don_idle;
    ip.don_fault = c->don_fault;
    return ip;
}

// rule C8: every driver runs its BOUNDED instantiation when the context's distance bounds anything (after icp_setup, which
// sizes d_ncorr)
IcpBound icp_bound(const cd_context* c) {
    IcpBound b;
    b.d2_max = c->icp_d2_max;
    b.bounded = c->icp_bounded;
    b.ncorr = c->d_ncorr;
    return b;
}

// after the host synchronise of the driver that ended the stage: the launch time (ev[5] -> ev[6]) and the point pairs tested
void icp_finish(cd_context* c, int ncl, long long* pair_tests) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, c->ev[5], c->ev[6]);
    c->timing.icp_kernel_ms = ms;
    if (pair_tests) {
        long long tot = 0;
        for (int k = 0; k < ncl; ++k)
            if (c->h_st[2 * k].status == CD_OK) tot += (long long)c->h_cl[k].n * c->h_cl[k].tpl_m * (c->h_st[2 * k].iters + 1);
        *pair_tests = tot;
    }
}

// k_icp_lat over the clusters whose template is a lattice; on a mixed batch the states come back for the drivers below.
int icp_run_lat(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, n_lat = pl.n_lat, lat_max_n = pl.lat_max_n;
    // the clusters of the launch, largest first
    int no = 0;
    for (int k = 0; k < ncl; ++k) if (pl.in_lat[(size_t)k]) c->h_order[no++] = k;
    std::stable_sort(c->h_order.get(), c->h_order + no, [&](int a, int b) { return c->h_cl[a].n > c->h_cl[b].n; });
    if (!pl.lat_direct) HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)no, hipMemcpyHostToDevice));
    // Shape of the launch (k_icp_lat.hip): clusters per workgroup x waves per cluster.  A call that has the GPU to itself wants
    // the launch short: one cluster per workgroup, four waves each when there are clusters enough to fill the chip twice that way,
    // eight or sixteen for fewer or very large clusters (one frame; config 5's thousands of points).  With other batches in
    // flight the chip is full anyway: four clusters per workgroup, two waves each, pay the single-lane solve of a round once
    // for the four (measured on config 3, seven in flight, profiles/r05_lat_shapes.txt: 1x4 145-146 k, 4x2 149-151 k, 8x2 146 k,
    // 4x4 139 k, 4x1 131 k frames/s; alone 1x4 1.34 ms, 1x8 1.30, 4x2 2.2, 4x1 2.8).  CUBOID_LAT_SHAPE=cpw,wpc[,clusters per slot].
    const bool busy = g_batches_in_flight[c->device & (MAX_DEVICES - 1)].load() >= 3;
    int cpw = 1, wpc = n_lat >= 768 ? 4 : (n_lat >= 96 ? 8 : 16), per_slot = 1;   // (end of round 5, 522 clusters alone: 1x4 1.17 ms, 1x8 1.10, 1x16 1.53, 2x4 1.27)
    if (lat_max_n > 16384) wpc = 16;
    else if (lat_max_n > 4096) wpc = std::max(wpc, 8);
    if (busy && n_lat >= 256 && lat_max_n <= 8192) { cpw = 4; wpc = 2; }
    if (c->lat_shape[0] > 0) { cpw = c->lat_shape[0]; wpc = std::max(1, c->lat_shape[1]); per_slot = std::max(1, c->lat_shape[2]); }
    const int n_wg = std::max(1, (n_lat + cpw * per_slot - 1) / (cpw * per_slot));
    GateHold lat_hold;   // (CUBOID_ICP_CONCURRENT: at most that many contexts between this launch and its completion)
    if (c->icp_concurrent > 0) lat_hold.enter(&g_icp_gate[c->device & (MAX_DEVICES - 1)], c->icp_concurrent);
    if (!pl.pre_zeroed) HIPCHK(c, hipMemsetAsync(c->d_queue, 0, 2 * sizeof(int), c->stream));   // head of the cluster queue, count of finished workgroups
    if (pl.lat_direct) std::memset(c->h_accf, 0, sizeof(unsigned long long) * ((size_t)ncl + 1));   // (what the zeroed device array used to bring back for clusters the kernel skips)
    if (pl.lat_direct)
        LAUNCH(c, launch_icp_lat(c->stream, n_lat, cpw, wpc, n_wg, c->h_order, c->h_cl, c->h_st, c->h_accf, c->d_lat, c->d_src, c->d_src0, c->d_queue, c->d_accf + ncl, c->h_accf + ncl, ip, icp_bound(c)));
    else
        LAUNCH(c, launch_icp_lat(c->stream, n_lat, cpw, wpc, n_wg, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_lat, c->d_src, c->d_src0, c->d_queue, c->d_accf + ncl, nullptr, ip, icp_bound(c)));
    c->timing.icp_kernel_launches = 1;
    c->timing.icp_regime = (cpw << 16) | std::min(n_wg, 0xffff);
    if (n_lat < pl.n_live) {   // mixed batch
        HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    if (!pl.lat_direct) {
        XferBatch xb(c);   // (one launch)
        xb.add(c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost);
        xb.add(c->h_accf, c->d_accf, sizeof(unsigned long long) * ((size_t)ncl + 1), hipMemcpyDeviceToHost);
        HIPCHK(c, xb.flush());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->timing.icp_wave_ms = (float)((double)c->h_accf[ncl] / 1.0e5);   // 100 MHz ticks x waves -> wave-milliseconds
    *done = true;
    return CD_OK;
}

// The template groups of a several-template batch (plan.grouped_pipe): k_icp_pipe and k_icp_pipe_big side by side; the stage
// is finished when no cluster is left for the sliced driver.
int icp_run_grouped(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl;
    // items of `order`: the pipe groups one after the other (those of k_icp_pipe first, then those of k_icp_pipe_big),
    // each largest cluster first.  The two kernels are launched side by side (second stream): their workgroups share the
    // chip, every group gets workgroups in proportion to its points (a query against a template in global memory
    // counted BIG_WEIGHT times), at least one, no more than it has clusters.
    const int wg_cap = pl.wg_cap;
    // (while every problem can have a workgroup of its own the launch lasts as long as its longest cluster, and those are the
    // global-memory ones: 4; with more problems than workgroups it is their throughput that counts, 1.6 x the LDS kernel's
    // cost per workgroup plus the longer tail: 2 - config 5 at 8 frames per batch 4 > 2 by 5 %, at 64 frames 2 > 4 by 6 %)
    int live_all = 0;
    for (const TplGroup& g : pl.groups) if (g.kind) live_all += g.live;
    const long long BIG_WEIGHT = c->icp_big_weight > 0 ? c->icp_big_weight : (live_all <= wg_cap ? 4 : 2);
    const int cpw = std::max(1, c->icp_cpw);   // (0 = default: a group may have as many workgroups as clusters)
    // (template groups keep two clusters in flight per workgroup whatever the regime: every group has its share of the
    // workgroups and its own queue already, and four slots measure 3-7 % slower on config 5)
    IcpParams ipg = ip;
    if (c->icp_slots <= 0) ipg.pipe_slots = std::min(2, CD_PIPE_SLOTS);
    int* tab = c->h_wgtab;   // pinned: the copy below is asynchronous
    int ntab = 0;
    long long pts_all = 0;
    int npg = 0;
    for (const TplGroup& g : pl.groups) if (g.kind && g.live > 0) { pts_all += g.pts * (g.kind == 2 ? BIG_WEIGHT : 1); ++npg; }
    int no = 0, gq = 0, n_wg = 0, wg_of[3] = {0, 0, 0}, tab_of[3] = {0, 0, 0};
    for (int kind = 1; kind <= 2; ++kind) {
        tab_of[kind] = ntab;
        for (const TplGroup& g : pl.groups) {
            if (g.kind != kind || g.live == 0) continue;
            const int b = no;
            for (int k = g.beg; k < g.end; ++k) if (c->h_cl[k].n >= 3) c->h_order[no++] = k;
            std::stable_sort(c->h_order + b, c->h_order + no, [&](int x, int y) { return c->h_cl[x].n > c->h_cl[y].n; });
            int share = (int)((long long)wg_cap * g.pts * (kind == 2 ? BIG_WEIGHT : 1) / std::max(pts_all, 1ll));
            share = std::max(1, std::min(share, std::min((g.live + cpw - 1) / cpw, wg_cap - n_wg - (npg - 1 - gq))));
            for (int w = 0; w < share && ntab + 3 <= 3 * 1024; ++w) { tab[ntab++] = b; tab[ntab++] = no; tab[ntab++] = gq; }
            n_wg += share;
            wg_of[kind] += share;
            ++gq;
        }
    }
    HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)no, hipMemcpyHostToDevice));
    HIPCHK(c, xfer(c, c->d_wgtab, tab, sizeof(int) * (size_t)ntab, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_queue, 0, sizeof(int) * 16, c->stream));   // one queue head per group
    // the LDS-template launch goes to the context's stream (stream3 with icp_lowprio), the global-template launch beside it
    hipStream_t s1 = c->icp_lowprio ? c->stream3 : c->stream;
    hipStream_t s2 = (c->icp_lowprio || (wg_of[1] > 0 && wg_of[2] > 0)) ? c->stream2 : c->stream;
    if (s1 != c->stream || s2 != c->stream) {   // everything uploaded so far is visible to the side streams
        HIPCHK(c, hipEventRecord(c->ev2[0], c->stream));
        if (s1 != c->stream) HIPCHK(c, hipStreamWaitEvent(s1, c->ev2[0], 0));
        if (s2 != c->stream) HIPCHK(c, hipStreamWaitEvent(s2, c->ev2[0], 0));
    }
    if (wg_of[1] > 0)
        LAUNCH(c, launch_icp_pipe(s1, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid, c->d_tcell, c->d_src, c->d_src0, c->d_nn,
                        c->d_queue, wg_of[1], c->d_wgtab + tab_of[1], ipg, icp_bound(c)));
    if (wg_of[2] > 0)
        LAUNCH(c, launch_icp_pipe_big(s2, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tplk, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid,
                            c->d_super, c->d_tcell, c->d_src, c->d_src0, c->d_nn, c->d_queue, wg_of[2], c->d_wgtab + tab_of[2], ipg, icp_bound(c)));
    if (s1 != c->stream && wg_of[1] > 0) {
        HIPCHK(c, hipEventRecord(c->ev2[2], s1));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[2], 0));
    }
    if (s2 != c->stream && wg_of[2] > 0) {
        HIPCHK(c, hipEventRecord(c->ev2[1], s2));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[1], 0));
    }
    c->timing.icp_kernel_launches = 1;
    c->timing.icp_regime = (ipg.pipe_slots << 16) | n_wg;
    if (pl.nwork > 0) {   // the other clusters take the sliced driver
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *done = true;
    return CD_OK;
}

// One launch in which every cluster runs its whole ICP in one workgroup (plan.whole_cluster): k_icp_pipe, k_icp_pipe_big or
// k_icp_cluster.  Always finishes the stage.
int icp_run_whole(cd_context* c, const IcpPlan& pl, IcpParams ip, bool* done) {
    const int ncl = pl.ncl;
    auto pipe_grid = [&](int n_items, int cap) {   // workgroups of the launch over n_items clusters
        if (c->icp_cpw > 0) return std::min((n_items + c->icp_cpw - 1) / c->icp_cpw, cap);
        if (!pl.crowded || n_items <= cap) return std::min(n_items, cap);
        return std::min(cap, std::max(32, (n_items / ip.pipe_slots + 16) / 32 * 32));
    };
    GateHold hold;   // (released on every path out of this function)
    if (c->icp_concurrent > 0) hold.enter(&g_icp_gate[c->device & (MAX_DEVICES - 1)], c->icp_concurrent);
    for (int k = 0; k < ncl; ++k) c->h_order[k] = k;
    std::stable_sort(c->h_order.get(), c->h_order + ncl, [&](int a, int b) { return c->h_cl[a].n > c->h_cl[b].n; });
    HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * ncl, hipMemcpyHostToDevice));
    const int wg_cap = pl.wg_cap;
    HIPCHK(c, hipMemsetAsync(c->d_queue, 0, sizeof(int), c->stream));   // head of the cluster queue
    hipStream_t si = c->icp_lowprio >= 2 ? c->stream3 : c->stream;
    if (pl.pipe_ok || pl.big_ok) {
        c->timing.icp_regime = (ip.pipe_slots << 16) | pipe_grid(ncl, wg_cap);
        // A launch that has the GPU to itself lets workgroups that run out of clusters wait and take over running ones
        // (k_icp.hip, "hand-over of running clusters"): the launch is as long as its slowest workgroup, and the bench batch's
        // slowest runs 25 % over the average.  With other calls in flight a waiting workgroup would sit on a CU their
        // kernels could use, and what counts there is the CU-time a batch costs, which hand-overs do not lower.
        const bool alone = g_batches_in_flight[c->device & (MAX_DEVICES - 1)].load() <= 1;
        ip.donate = (c->icp_donate < 0 ? (alone && ncl > pipe_grid(ncl, wg_cap)) : c->icp_donate != 0) ? 1 : 0;
        if (ip.donate) HIPCHK(c, hipMemsetAsync(c->d_don, 0, sizeof(int) * (size_t)(DON_BOX + DON_CAP), c->stream));
    }
    if (si != c->stream) {   // (after the control block was zeroed on c->stream: the launch on `si` must see it zeroed - ADVICE r4)
        HIPCHK(c, hipEventRecord(c->ev2[0], c->stream));
        HIPCHK(c, hipStreamWaitEvent(si, c->ev2[0], 0));
    }
    if (pl.pipe_ok)
        LAUNCH(c, launch_icp_pipe(si, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid, c->d_tcell, c->d_src, c->d_src0, c->d_nn,
                        c->d_queue, pipe_grid(ncl, wg_cap), nullptr, ip, icp_bound(c)));
    else if (pl.big_ok)
        LAUNCH(c, launch_icp_pipe_big(si, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tplk, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid, c->d_super, c->d_tcell,
                            c->d_src, c->d_src0, c->d_nn, c->d_queue, pipe_grid(ncl, wg_cap), nullptr, ip, icp_bound(c)));
    else
        LAUNCH(c, launch_icp_cluster(si, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tlo, c->d_thi, c->d_grid, c->d_tcell, c->d_src, c->d_src0, c->d_nn,
                           c->d_queue, wg_cap, ip, icp_bound(c)));
    if (si != c->stream) {
        HIPCHK(c, hipEventRecord(c->ev2[2], si));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[2], 0));
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    c->timing.icp_kernel_launches = 1;
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    if (ip.donate) HIPCHK(c, xfer(c, c->h_ctl + 8, c->d_don, sizeof(int) * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *done = true;   // (also when the hand-over check below fails the call: icp_kernel_ms is reported)
    if (ip.donate) {
        const int* w = c->h_ctl + 8;   // (copied with the records above)
        c->timing.icp_handovers = w[DON_HEAD];
        // every cluster of the launch was finished by somebody, and every mailbox entry that was written was taken
        if (w[DON_ERR] != 0 || w[DON_FINISHED] != ncl || w[DON_HEAD] != std::min(w[DON_TAIL], DON_CAP)) {
            c->timing.icp_handover_lost = 1;
            std::snprintf(c->err, sizeof(c->err), "ICP hand-over lost a cluster: %d of %d clusters finished, %d entries published, %d taken, error word %d",
                          w[DON_FINISHED], ncl, w[DON_TAIL], w[DON_HEAD], w[DON_ERR]);
            return CD_ERR_DEVICE;
        }
        if (std::getenv("CUBOID_DEBUG"))
            std::fprintf(stderr, "cuboid_hip: hand-overs: %d published, %d taken, %d clusters finished of %d, waiting balance %d\n", w[DON_TAIL], w[DON_HEAD], w[DON_FINISHED], ncl, w[DON_AVAIL]);
    }
    return CD_OK;
}

// Few clusters: ONE persistent launch runs every iteration and the fitness pass (k_icp_persist: grid barrier per
// iteration instead of two kernel launches).  Needs all its workgroups resident together; a barrier that does not
// complete in time makes it give up, and the sliced driver takes over from the initial state (not done).
int icp_run_persist(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, nwork = pl.nwork;
    // (with other contexts at work - BatchPipeline - their persistent kernels hold the CUs this launch's grid barrier needs:
    // it would wait, give up and hand over; go straight to the multi-launch loop then)
    const bool siblings = g_calls_in_flight[c->device & (MAX_DEVICES - 1)].load() > 1;
    if (nwork == 0 || !c->icp_persist || (siblings && c->icp_persist != 2)) return CD_OK;
    const int G = std::min(nwork, pl.wg_cap);
    // measured against the multi-launch loop: 1 frame 1.50 / 1.78 ms, 4 frames 1.94 / 2.36, 8 frames 3.04 / 2.66 - with many
    // clusters the launch lasts as long as the slowest one while finished workgroups wait at the barriers, and a workgroup
    // with several items solves for each of them in turn
    if (ncl > 8 || nwork > G) return CD_OK;
    int n_open = 0;
    for (int k = 0; k < ncl; ++k) if (c->h_cl[k].tile0 < (k + 1 < ncl ? c->h_cl[k + 1].tile0 : nwork)) ++n_open;
    // d_queue[4] barrier counter, [5] abort flag, [6..9] clusters closed per iteration slot (k_icp_persist's exit test)
    int* ctl = c->h_ctl;
    for (int i = 0; i < 8; ++i) ctl[i] = 0;
    ctl[1] = c->icp_persist == 2 ? 1 : 0;
    HIPCHK(c, xfer(c, c->d_queue + 4, ctl, sizeof(int) * 6, hipMemcpyHostToDevice));
    LAUNCH(c, launch_icp_persist(c->stream, nwork, G, ip.max_iter + 3, c->d_work, c->d_cl, c->d_st, c->d_acc, c->d_accf, c->d_tplk, c->d_tlok, c->d_thik, c->d_grid,
                       c->d_src, c->d_src0, c->d_nn, c->d_d2, pl.qslice, (unsigned*)(c->d_queue + 4), c->d_queue + 5, n_open, c->d_queue + 6, ip, icp_bound(c)));
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    HIPCHK(c, xfer(c, ctl + 8, c->d_queue + 5, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    c->st_init.assign(c->h_st.get(), c->h_st + 2 * (size_t)ncl);   // in case the launch gives up (no reallocation after the first call)
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!ctl[8]) {   // (the abort flag: raised when the launch gave up)
        c->timing.icp_kernel_launches = 1;
        *done = true;
        return CD_OK;
    }
    c->persist_gave_up += 1;
    c->timing.icp_persist_gave_up += 1;
    if (std::getenv("CUBOID_DEBUG")) std::fprintf(stderr, "cuboid_hip: persistent ICP launch gave up at a grid barrier, running the multi-launch loop\n");
    // start over: initial states, zero sums, the source points as extracted (the launch transformed them in place)
    std::memcpy(c->h_st, c->st_init.data(), sizeof(IcpState) * 2 * (size_t)ncl);
    HIPCHK(c, xfer(c, c->d_st, c->h_st, sizeof(IcpState) * 2 * ncl, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_acc, 0, sizeof(unsigned long long) * 48 * (size_t)ncl, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_accf, 0, sizeof(unsigned long long) * (size_t)ncl, c->stream));
    if (c->icp_bounded) HIPCHK(c, hipMemsetAsync(c->d_ncorr, 0, sizeof(uint32_t) * 3 * (size_t)ncl, c->stream));
    long long span = 0;
    for (int k = 0; k < ncl; ++k) span = std::max(span, (long long)c->h_cl[k].src_off + c->h_cl[k].n);
    HIPCHK(c, hipMemcpyAsync(c->d_src, c->d_src0, sizeof(float4) * (size_t)span, hipMemcpyDeviceToDevice, c->stream));
    if (pl.guess_mode == CD_GUESS_CLUSTER)   // (the states just uploaded start from the identity again)
        if (int e = launch_cluster_guesses(c, ncl)) return e;
    if (pl.guess_mode != CD_GUESS_NONE)
        LAUNCH(c, launch_icp_apply_guess(c->stream, ncl, pl.max_n, c->d_cl, c->d_guess, guess_indexing(pl.guess_mode), c->d_src0, c->d_src));
    return CD_OK;
}

// The multi-launch loop over the work list, then the fitness pass.  Always finishes the stage.
int icp_run_sliced(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, nwork = pl.nwork, max_launch = ip.max_iter + 3;
    // The iteration kernel walks an ACTIVE work list (d_work2) that the host re-packs at every
    // completion poll, dropping the clusters that have converged; the full list (d_work) is kept for
    // the fitness pass.  A cluster whose state shows done in either parity slot has already had its
    // final transform applied, so it needs no further work items (k_icp_solve alone keeps its state).
    int it = 0, nactive = nwork;
    std::memcpy(c->h_work2, c->h_work, sizeof(IcpWork) * (size_t)std::max(nwork, 1));
    HIPCHK(c, xfer(c, c->d_work2, c->h_work2, sizeof(IcpWork) * (size_t)std::max(nwork, 1), hipMemcpyHostToDevice));
    int group = 8;
    while (nwork > 0 && it < max_launch) {
        const int g = std::min(group, max_launch - it);
        for (int q = 0; q < g; ++q) LAUNCH(c, launch_icp_iter(c->stream, it++, nactive, ncl, c->d_work2, c->d_cl, c->d_st, c->d_acc, c->d_tplk, c->d_tlok, c->d_thik, c->d_grid, c->d_src, c->d_nn, c->d_d2, pl.qslice, c->d_queue, c->n_cu, ip, icp_bound(c)));
        HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bool all = true;
        int na = 0;
        for (int w = 0; w < nwork; ++w) {
            const int k = c->h_work[w].cluster;
            if (!(c->h_st[2 * k].done || c->h_st[2 * k + 1].done)) c->h_work2[na++] = c->h_work[w];
        }
        for (int k = 0; k < ncl && all; ++k) all = c->h_st[2 * k].done && c->h_st[2 * k + 1].done;
        if (all) break;
        if (na != nactive) {
            nactive = na;
            if (na > 0) HIPCHK(c, xfer(c, c->d_work2, c->h_work2, sizeof(IcpWork) * (size_t)na, hipMemcpyHostToDevice));
        }
        group = 16;
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));   // (before the fitness pass)
    c->timing.icp_kernel_launches = it;
    LAUNCH(c, launch_icp_fitness(c->stream, nwork, c->d_work, c->d_cl, c->d_st, 0, c->d_accf, c->d_tplk, c->d_tlok, c->d_thik, c->d_grid, c->d_src0, c->d_nn, c->d_d2, pl.qslice));
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *done = true;
    return CD_OK;
}

// S6.  clusters described by h_cl[0..ncl) (src_off relative to d_src/d_src0).  Fills h_st / h_accf.
int stage_icp(cd_context* c, int ncl, const cd_params* p, long long* pair_tests) {
    c->timing.icp_kernel_launches = 0;
    c->timing.icp_kernel_ms = 0.f;
    if (pair_tests) *pair_tests = 0;
    if (ncl <= 0) return CD_OK;
    IcpPlan pl;
    int st = plan_icp(c, ncl, p, &pl);
    if (!st) st = icp_setup(c, p, &pl);
    if (st) return st;
    const IcpParams ip = icp_params(c, p, &pl.crowded);
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    bool done = false;
    if (pl.n_lat > 0) st = icp_run_lat(c, pl, ip, &done);
    if (!st && !done && pl.grouped_pipe) st = icp_run_grouped(c, pl, ip, &done);
    if (!st && !done && pl.whole_cluster) st = icp_run_whole(c, pl, ip, &done);
    if (!st && !done) st = icp_run_persist(c, pl, ip, &done);
    if (!st && !done) st = icp_run_sliced(c, pl, ip, &done);
    if (done) icp_finish(c, ncl, pair_tests);
    return st;
}

void fill_cluster_result(const cd_context* c, int k, const cd_params* p, cd_cluster_result* r) {
    const IcpState& st = c->h_st[2 * k];
    const IcpCluster& cl = c->h_cl[k];
    std::memset(r, 0, sizeof(*r));
    r->size = cl.n;
    r->iterations = st.iters;
    r->converged = st.converged;
    std::memcpy(r->T, st.Tfinal, 64);
    r->fitness = st.status == CD_OK ? hm::unfix(c->h_accf[k], FIX_SHIFT_D2) / (double)cl.n : std::numeric_limits<double>::max();
    r->accepted = (r->converged && r->fitness < p->icp_accept_fitness) ? 1 : 0;
    double Td[16];
    for (int i = 0; i < 16; ++i) Td[i] = (double)st.Tfinal[i];
    if (!hm::mat4_inverse(Td, r->pose))
        for (int i = 0; i < 16; ++i) r->pose[i] = std::numeric_limits<double>::quiet_NaN();
}

int upload_points(cd_context* c, const void* pts, size_t stride, int n, float4* dst) {
    // host (stride) -> device float4 via the staging buffer
    if (n <= 0) return CD_OK;
    std::vector<float4> tmp((size_t)n);
    const char* b = (const char*)pts;
    for (int i = 0; i < n; ++i) {
        float v[3];
        std::memcpy(v, b + (size_t)i * stride, 12);
        tmp[i] = make_float4(v[0], v[1], v[2], 0.f);
    }
    HIPCHK(c, hipMemcpyAsync(dst, tmp.data(), sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CD_OK;
}

int check_params(cd_context* c, const cd_params* p) {
    if (!p) return fail(c, CD_ERR_INVALID_ARG, "params is NULL");
    if (!(p->leaf_size > 0.f)) return fail(c, CD_ERR_INVALID_ARG, "leaf_size must be > 0");
    if (p->plane_max_iterations < 0 || p->plane_max_iterations > 1000) return fail(c, CD_ERR_INVALID_ARG, "plane_max_iterations must be in [0,1000]");
    if (p->template_slot < -1 || p->template_slot >= CD_MAX_TEMPLATES) return fail(c, CD_ERR_INVALID_ARG, "template_slot out of range");
    if (!(p->cluster_tolerance > 0.0)) return fail(c, CD_ERR_INVALID_ARG, "cluster_tolerance must be > 0");
    if (p->plane_model < CD_PLANE || p->plane_model > CD_PLANE_PARALLEL) return fail(c, CD_ERR_INVALID_ARG, "plane_model out of range");
    if (p->icp_use_guess < CD_GUESS_NONE || p->icp_use_guess > CD_GUESS_CLUSTER) return fail(c, CD_ERR_INVALID_ARG, "icp_use_guess out of range");
    if (p->icp_use_guess == CD_GUESS_PARAMS)
        for (int i = 0; i < 16; ++i) if (!std::isfinite(p->icp_guess[i])) return fail(c, CD_ERR_INVALID_ARG, "icp_guess holds a non-finite value");
    return CD_OK;
}

// ---- batched surface-normal estimation (sne.cpp:167-234 over F frames: cd_surface_batch, CD_GUESS_SURFACE) ----------------
// The three constrained fits run over every frame at once: round i is stage_plane + stage_extract on each frame's current
// cloud, k_surface_centroid sums the plane points, and the leftover cloud (ExtractIndices(negative = invert), what S3 writes to
// its object buffer with extract_negative = invert) is the next round's cloud; a frame whose fit fails drops out.  The stages
// run on the surface stage's own buffers: SurfaceBuffers swaps them in for its lifetime.

int ensure_surface(cd_context* c, size_t pitch) {   // (the per-frame arrays at the context's capacity, the clouds as needed)
    const size_t F = (size_t)c->F, need = F * std::max<size_t>(pitch, 1);
    GROW(c, d_sfs, F); GROW(c, h_sfs, F);
    GROW(c, d_smodel, F); GROW(c, h_smodel, F);
    GROW(c, d_shave, F); GROW(c, h_shave, F);
    GROW(c, d_sactive, F); GROW(c, h_sactive, F);
    GROW(c, d_ssum, 3 * F); GROW(c, h_ssum, 3 * F);
    GROW(c, d_spts[0], need); GROW(c, d_spts[1], need); GROW(c, d_sidx, need);
    return CD_OK;
}

// For its lifetime the S2/S3 stage drivers work on the surface stage's buffers: FrameStates, models, have / active flags,
// d_vox = the current clouds (d_spts[0]), d_obj = the next (d_spts[1]), d_plane_idx; row pitch `pitch` points.  Its own
// scratch fills are done by the stages (batch_zeroed off); everything is put back on every way out.
struct SurfaceBuffers {
    cd_context* c;
    int N, T;
    bool zeroed;
    SurfaceBuffers(cd_context* ctx, int pitch) : c(ctx), N(ctx->N), T(ctx->T), zeroed(ctx->batch_zeroed) {
        swap_all();
        c->N = pitch;
        c->T = (pitch + TILE - 1) / TILE;
        c->batch_zeroed = false;
    }
    ~SurfaceBuffers() {
        swap_all();
        c->N = N;
        c->T = T;
        c->batch_zeroed = zeroed;
    }
    void swap_all() {
        std::swap(c->d_fs, c->d_sfs); std::swap(c->h_fs, c->h_sfs);
        std::swap(c->d_model, c->d_smodel); std::swap(c->h_model, c->h_smodel);
        std::swap(c->d_have, c->d_shave); std::swap(c->h_have, c->h_shave);
        std::swap(c->d_active, c->d_sactive); std::swap(c->h_active, c->h_sactive);
        std::swap(c->d_vox, c->d_spts[0]); std::swap(c->d_obj, c->d_spts[1]);
        std::swap(c->d_plane_idx, c->d_sidx);
    }
};

// in: the clouds in d_spts[0] (rows of `pitch` points), count[f] points each; axes: 3 floats per frame; run[f] = 0: frame f is
// not fitted (status CD_ERR_NO_MODEL, zero record).  q: the fit parameters (threshold, probability) as cd_surface_frame takes them.
int stage_surface(cd_context* c, int F, int pitch, const std::vector<int>& count, const float* axes, const std::vector<char>& run,
                  int invert, const cd_params* p, cd_surface_frame_result* res, int32_t* status) {
    for (int f = 0; f < F; ++f) {
        std::memset(&res[f], 0, sizeof(res[f]));
        status[f] = run[(size_t)f] ? CD_OK : CD_ERR_NO_MODEL;
    }
    const float thr = hm::fold_ge(p->plane_distance_threshold);
    std::vector<int> n(count);
    {
        SurfaceBuffers sb(c, pitch);
        for (int i = 0; i < 3; ++i) {   // sne.cpp:183-197
            cd_params q = *p;
            q.plane_model = i == 0 ? CD_PLANE_PERPENDICULAR : CD_PLANE_PARALLEL;
            q.plane_eps_angle = 0.1;                       // sne.cpp:123
            q.plane_optimize = 1;                          // sne.cpp:118
            q.plane_max_iterations = 1000;                 // sne.cpp:125
            q.extract_negative = invert ? 1 : 0;           // S3's object output = the leftover cloud
            q.crop2_enable = 0;
            q.bbox_enable = 0;
            bool any = false;
            for (int f = 0; f < F; ++f) {   // a fresh FrameState per fit, as load_as gives cd_surface_frame; frames out of the run stay idle
                FrameState& fs = c->h_fs[f];
                std::memset(&fs, 0, sizeof(fs));
                const bool live = status[f] == CD_OK;
                fs.status = live ? CD_OK : CD_ERR_INVALID_ARG;   // (stage_plane fits the frames whose status is OK or NO_MODEL)
                fs.n_v = live ? n[(size_t)f] : 0;
                any = any || live;
            }
            if (!any) break;
            HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState) * F, hipMemcpyHostToDevice));
            std::vector<int> iters;
            int st = stage_plane(c, F, &q, iters, nullptr, axes);
            if (st) return st;
            for (int f = 0; f < F; ++f) {
                if (status[f] != CD_OK) continue;
                res[f].iterations[i] = iters[(size_t)f];
                if (!c->h_have[f]) status[f] = CD_ERR_NO_MODEL;
            }
            st = stage_extract(c, F, &q);
            if (st) return st;
            LAUNCH(c, launch_surface_centroid(c->stream, c->d_vox, pitch, F, c->d_fs, c->mirror_reads ? c->h_model : c->d_model,
                                              c->mirror_reads ? c->h_active : c->d_have, thr, invert, c->d_ssum + i, 3));
            st = sync_fs(c, F, c->mirror_writes && c->copy_kernels);   // n_o: the leftover clouds
            if (st) return st;
            for (int f = 0; f < F; ++f) {
                if (status[f] != CD_OK) continue;
                n[(size_t)f] = c->h_fs[f].n_o;
                const float4 m = c->h_model[f];   // (in fit order; sorted below)
                res[f].coeff[i][0] = m.x; res[f].coeff[i][1] = m.y; res[f].coeff[i][2] = m.z; res[f].coeff[i][3] = m.w;
            }
            std::swap(c->d_vox, c->d_obj);
        }
    }
    HIPCHK(c, xfer(c, c->h_ssum, c->d_ssum, sizeof(float4) * 3 * (size_t)F, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < F; ++f) {
        cd_surface_frame_result& r = res[f];
        if (status[f] != CD_OK) {   // (a failed fit leaves the iterations of the fits run so far and nothing else)
            std::memset(r.coeff, 0, sizeof(r.coeff));
            continue;
        }
        float normals[3][4], mids[3][4];
        int counts[3];
        for (int i = 0; i < 3; ++i) {
            const float4 sm = c->h_ssum[3 * (size_t)f + i];
            std::memcpy(&counts[i], &sm.w, 4);
            const float cnt = (float)counts[i];   // pcl::compute3DCentroid: the sums / the count
            mids[i][0] = sm.x / cnt; mids[i][1] = sm.y / cnt; mids[i][2] = sm.z / cnt; mids[i][3] = 0.f;
            for (int a = 0; a < 4; ++a) normals[i][a] = r.coeff[i][a];
        }
        for (int i = 0; i < 3; ++i)   // sne.cpp:199-212, as cd_surface_frame
            for (int j = i; j < 3; ++j)
                if (counts[i] < counts[j]) {
                    std::swap(counts[i], counts[j]);
                    for (int a = 0; a < 4; ++a) { std::swap(normals[i][a], normals[j][a]); std::swap(mids[i][a], mids[j][a]); }
                }
        hm::surface_frame(normals, mids, r.Rt);
        for (int i = 0; i < 3; ++i) {
            r.n_points[i] = counts[i];
            for (int a = 0; a < 4; ++a) { r.coeff[i][a] = normals[i][a]; r.midpoint[i][a] = mids[i][a]; }
        }
    }
    return CD_OK;
}

// CD_GUESS_SURFACE: the surface fit of every frame that has a ground plane, on its objects cloud (d_obj, n_o), table normal =
// its plane, invert = 1, the context's threshold -> c->last_surface*; rule C9 -> c->surface_guess (identity where the fit
// fails); (*flagged)[f] = 1 where the guess came from the fit
int surface_guesses(cd_context* c, int F, const cd_params* p, std::vector<char>* flagged) {
    std::vector<int> count((size_t)F, 0);
    std::vector<char> run((size_t)F, 0);
    std::vector<float> axes(3 * (size_t)F, 0.f);
    int pitch = 1;
    for (int f = 0; f < F; ++f) {
        if (!c->h_have[f]) continue;
        run[(size_t)f] = 1;
        count[(size_t)f] = c->h_fs[f].n_o;
        pitch = std::max(pitch, count[(size_t)f]);
        axes[3 * (size_t)f] = c->h_model[f].x; axes[3 * (size_t)f + 1] = c->h_model[f].y; axes[3 * (size_t)f + 2] = c->h_model[f].z;
    }
    int st = ensure_surface(c, (size_t)pitch);
    if (st) return st;
    LAUNCH(c, launch_surface_load(c->stream, c->d_obj, sizeof(float4), sizeof(float4) * (size_t)c->N, FS_FIELD(c, n_o), FS_PITCH, pitch, pitch, F, c->d_spts[0]));
    cd_params q = *p;
    q.plane_distance_threshold = c->surface_thr;
    c->last_surface.assign((size_t)F, cd_surface_frame_result());
    c->last_surface_status.assign((size_t)F, CD_ERR_NO_MODEL);
    st = stage_surface(c, F, pitch, count, axes.data(), run, 1, &q, c->last_surface.data(), c->last_surface_status.data());
    if (st) return st;
    c->surface_guess.assign(16 * (size_t)F, 0.f);
    flagged->assign((size_t)F, 0);
    for (int f = 0; f < F; ++f) {
        float* g = c->surface_guess.data() + 16 * (size_t)f;
        for (int i = 0; i < 4; ++i) g[5 * i] = 1.f;
        float h[16];
        if (c->last_surface_status[(size_t)f] == CD_OK && cd_surface_guess(c->last_surface[(size_t)f].Rt, h) == CD_OK) {
            std::memcpy(g, h, sizeof(h));
            (*flagged)[(size_t)f] = 1;
        }
    }
    return CD_OK;
}

// depth images of a batch on the device, deprojected into the records d_frames of process_batch_impl (k_depth.hip)
struct DepthJob {
    const cd_depth_camera* cam;
    const uint16_t* depth;
    const uint8_t* color;   // nullptr: no colour
    const cd_color_camera* ccam = nullptr;   // a mapped call (rule C12, k_texture.hip): `color` is ccam->width x ccam->height per frame
};

TextureParams texture_params(const cd_depth_camera* cam, const cd_color_camera* cc) {
    TextureParams tp;
    tp.fx = cam->fx; tp.fy = cam->fy; tp.cx = cam->cx; tp.cy = cam->cy; tp.depth_scale = cam->depth_scale;
    tp.cfx = cc->fx; tp.cfy = cc->fy; tp.ccx = cc->cx; tp.ccy = cc->cy;
    for (int i = 0; i < 9; ++i) tp.R[i] = cc->R[i];
    for (int i = 0; i < 3; ++i) tp.t[i] = cc->t[i];
    tp.cw = cc->width; tp.ch = cc->height;
    tp.keep = cc->no_texture == CD_NOTEX_KEEP;
    return tp;
}

// the deprojection of a depth call into its records: rule C7 for registered images, rule C12 for a mapped call
void launch_depth_job(hipStream_t s, const DepthJob* dj, int F, float4* out) {
    if (dj->ccam)
        launch_texture_map(s, dj->depth, dj->color, dj->cam->width, dj->cam->height, F, texture_params(dj->cam, dj->ccam), out);
    else
        launch_deproject(s, dj->depth, dj->color, dj->cam->width, dj->cam->height, F, dj->cam->fx, dj->cam->fy, dj->cam->cx, dj->cam->cy,
                         dj->cam->depth_scale, out);
}

// ---- colour gate (rule C10, k_color.hip) ---------------------------------------------------------------------------------------
static_assert(sizeof(ColorRecord) == sizeof(cd_color_bbox) && offsetof(ColorRecord, rect) == 0 && offsetof(cd_color_bbox, rect) == 0, "the kernel's record is cd_color_bbox");
int check_color_params(cd_context* c, const cd_color_gate_params* g) {
    if (g->h_lo_max < 0 || g->h_lo_max > 179 || g->h_hi_min < 0 || g->h_hi_min > 179) return fail(c, CD_ERR_INVALID_ARG, "colour gate: the H bounds must be in 0 .. 179");
    if (g->s_min < 0 || g->s_min > 255 || g->v_min < 0 || g->v_min > 255) return fail(c, CD_ERR_INVALID_ARG, "colour gate: the S and V minima must be in 0 .. 255");
    if (g->margin < 0) return fail(c, CD_ERR_INVALID_ARG, "colour gate: the margin must not be negative");
    return CD_OK;
}

// the rectangles of F rgb8 images (device-resident, W x H each) into d_crec / d_cstatus, and on into their pinned mirrors
// (valid after the next synchronisation of the context's stream)
int stage_color(cd_context* c, const uint8_t* d_rgb, int W, int H, int F, const cd_color_gate_params* g) {
    const size_t px = (size_t)W * H;
    if (c->d_clabel.capacity() < px * F) GROW(c, d_clabel, std::max(px * F, std::min((size_t)c->N * c->F, (size_t)640 * 480 * c->F)));
    uint32_t* gmask = nullptr;
    if (!color_fits_lds(W, H)) {
        GROW(c, d_cmask, 2 * (size_t)((W + 31) / 32) * H * F);
        gmask = c->d_cmask;
    }
    const ColorGate cg{g->h_lo_max, g->h_hi_min, g->s_min, g->v_min, g->margin};
    LAUNCH(c, launch_color_bbox(c->stream, d_rgb, W, H, F, cg, c->d_ctab, gmask, c->d_clabel, px, c->d_crec, c->d_cstatus));
    HIPCHK(c, xfer(c, c->h_crec, c->d_crec, sizeof(ColorRecord) * (size_t)F, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_cstatus, c->d_cstatus, sizeof(int) * (size_t)F, hipMemcpyDeviceToHost));
    return CD_OK;
}

// after the synchronisation: a border walk that ran out of steps (cannot happen: the bound is every (pixel, direction) pair)
int color_status(cd_context* c, int F) {
    for (int f = 0; f < F; ++f)
        if (c->h_cstatus[f] != CD_OK) return fail(c, CD_ERR_CAPACITY, "colour gate: a border walk exceeded its step bound");
    return CD_OK;
}

// what a fused call's gate needs besides cd_params, checked before anything is copied or launched: `color` = the call is a
// depth call with registered colour images
int check_bbox_source(cd_context* c, const cd_params* p, int F, bool color) {
    if (!p || !p->bbox_enable || c->bbox_source == CD_BBOX_PARAMS) return CD_OK;
    if (c->bbox_source == CD_BBOX_PER_FRAME) {
        if (F > 0 && c->frame_rects.size() < 4 * (size_t)F) return fail(c, CD_ERR_INVALID_ARG, "bbox source CD_BBOX_PER_FRAME but cd_set_frame_bboxes holds fewer rectangles than the batch has frames");
        return CD_OK;
    }
    if (!color) return fail(c, CD_ERR_INVALID_ARG, "bbox source CD_BBOX_COLOR needs cd_process_depth_batch[_device] with CD_COLOR_RGB8 images");
    return CD_OK;
}

// ---- the fused batch call ---------------------------------------------------------------------------------------
// process_batch_impl, at the end of this section, is the sequence; the functions before it are its steps in the order it calls
// them.  Each says what it issues on the context's stream and which synchronisation it relies on.

// What a fused call sets on the context for its own duration only, put back on every way out: the rectangles its gate kernels
// read (call_rects) and the two marks of the zero launch that make the stages skip their own fills (batch_zeroed, fs_initialised).
struct BatchScope {
    cd_context* c;
    ~BatchScope() { c->call_rects = FrameRects{nullptr, 0}; c->batch_zeroed = false; c->fs_initialised = false; }
};

// Every scratch array the stages want zeroed, in ONE launch (a batch had ~14 fill kernels, each a stream operation of its own
// that queues behind the other contexts' kernels).  A scratch array that a stage expects zeroed is added to THIS list.
// Issues that launch and sets batch_zeroed / fs_initialised (BatchScope puts them back); relies on no synchronisation.
int zero_batch_scratch(cd_context* c, int F) {
    ZeroRegions zr;
    zr.n = 0;
    zr.fs = c->mirror_writes && c->copy_kernels ? c->d_fs : nullptr;   // (the crop stage then skips its upload of the initial FrameStates)
    zr.nfs = F;
    c->fs_initialised = zr.fs != nullptr;
    auto add = [&](void* ptr, size_t bytes) { zr.ptr[zr.n] = (uint32_t*)ptr; zr.words[zr.n] = bytes / 4; ++zr.n; };
    const size_t FT = (size_t)F * c->T;
    add(c->d_ticket, sizeof(int) * (size_t)F * TICKET_PITCH);
    add(c->d_tileA, sizeof(int) * FT);
    add(c->d_tileB, sizeof(int) * FT);
    add(c->d_tileC, sizeof(int) * FT);
    add(c->d_tile64, sizeof(unsigned long long) * FT);
    add(c->d_ghist, sizeof(uint32_t) * (size_t)F * SORT_MAX_PASSES_HOST * RADIX);
    add(c->d_counts, sizeof(int) * (size_t)F * MAX_HYP);
    add(c->d_sums, sizeof(unsigned long long) * 10 * (size_t)F);
    add(c->d_tileK, sizeof(int) * FT * KICP);
    add(c->d_acc, sizeof(unsigned long long) * 48 * (size_t)c->cl_cap);
    add(c->d_accf, sizeof(unsigned long long) * ((size_t)c->cl_cap + 1));
    add(c->d_queue, sizeof(int) * 16);
    LAUNCH(c, launch_zero_regions(c->stream, zr));
    c->batch_zeroed = true;
    return CD_OK;
}

// The call's stream work ahead of the crop stage, all of it after ev[0] and so inside stage [0] of the timing: the gate's
// per-frame rectangles (an upload for CD_BBOX_PER_FRAME, the colour stage for CD_BBOX_COLOR, whose records feed the gate on
// the device; call_rects then points at them), the deprojection of a depth call into d_frames, and the zero launch.
// Relies on no synchronisation and makes none.
int batch_prologue(cd_context* c, int gate_source, const void* d_frames, int F, const DepthJob* dj) {
    if (gate_source == CD_BBOX_PER_FRAME) {
        std::memcpy(c->h_rects, c->frame_rects.data(), sizeof(int32_t) * 4 * (size_t)F);
        HIPCHK(c, xfer(c, c->d_rects, c->h_rects, sizeof(int32_t) * 4 * (size_t)F, hipMemcpyHostToDevice));
        c->call_rects = FrameRects{c->d_rects, 4};
    } else if (gate_source == CD_BBOX_COLOR) {
        // (a mapped call: the raw colour images at their own size, so the rectangles are in colour pixels)
        int st = stage_color(c, dj->color, dj->ccam ? dj->ccam->width : dj->cam->width, dj->ccam ? dj->ccam->height : dj->cam->height, F, &c->color_prm);
        if (st) return st;
        c->call_rects = FrameRects{reinterpret_cast<const int32_t*>(c->d_crec.get()), (int32_t)(sizeof(ColorRecord) / sizeof(int32_t))};   // (rect is the record's first member)
    }
    if (dj) LAUNCH(c, launch_depth_job(c->stream, dj, F, (float4*)const_cast<void*>(d_frames)));
    return c->zero_once ? zero_batch_scratch(c, F) : CD_OK;
}

struct FrontStages {   // what the front stages leave for the frame records
    std::vector<int> iterations;     // RANSAC iterations of every frame (stage_plane)
    int rounds = 0;                  // hypothesis rounds of the plane stage
    std::vector<char> surface_flag;  // CD_GUESS_SURFACE: the frames whose guess came from their surface fit (empty otherwise)
};

struct BatchClusters {   // the host's table of a batch's clusters, frame-major (batch_clusters)
    std::vector<int> first;       // index of frame f's first cluster (F + 1 entries)
    std::vector<int> size, off;   // per cluster: its points; where its ICP source starts in the frame's segment of d_src0 / d_src
    std::vector<int> span;        // per frame: the points of all its clusters, i.e. of one copy of its ICP sources
    int ncl = 0, kmax = 0;        // clusters of the batch; of its fullest frame
    int rounds_k = 1;             // extraction rounds: ceil(kmax / KICP)
    long long points = 0;         // points of all clusters
    int To = 1;                   // tiles of the frame with the most object points (grid of the label kernels)
};

// Every cluster of every frame gets its ICP (opd.cpp:376-413).  The device extracts the ICP sources KICP clusters per frame at a
// time; frames with more than KICP clusters (rare) need further rounds, and the host needs their sizes.
// Fills the table from h_fs as stage_cluster_sync's synchronisation left it.  For each frame beyond KICP it issues one D2H copy
// of the sizes from d_sizes straight into cl->size and then synchronises the stream: cl->size is sized before the first copy and
// neither resized nor read until that synchronisation.  Ends with ensure_clusters for one ICP problem per cluster.
int batch_clusters(cd_context* c, int F, BatchClusters* cl) {
    cl->first.assign((size_t)F + 1, 0);
    int max_no = 0;   // (read again after the cluster stage's own synchronisation, not handed down from before it)
    for (int f = 0; f < F; ++f) {
        cl->first[(size_t)f] = cl->ncl;
        cl->ncl += c->h_fs[f].n_k;
        cl->kmax = std::max(cl->kmax, c->h_fs[f].n_k);
        max_no = std::max(max_no, c->h_fs[f].n_o);
    }
    cl->first[(size_t)F] = cl->ncl;
    cl->To = std::max(1, (max_no + TILE - 1) / TILE);
    cl->rounds_k = std::max(1, (cl->kmax + KICP - 1) / KICP);
    cl->size.assign((size_t)std::max(cl->ncl, 1), 0);
    cl->off.assign((size_t)std::max(cl->ncl, 1), 0);
    for (int f = 0; f < F; ++f) {
        const FrameState& s = c->h_fs[f];
        int* sz = cl->size.data() + cl->first[(size_t)f];
        if (s.n_k > KICP) HIPCHK(c, hipMemcpyAsync(sz, c->d_sizes + (size_t)f * c->N, sizeof(int) * (size_t)s.n_k, hipMemcpyDeviceToHost, c->stream));
        else for (int k = 0; k < s.n_k; ++k) sz[k] = s.ksize[k];
    }
    if (cl->rounds_k > 1) HIPCHK(c, hipStreamSynchronize(c->stream));
    cl->span.assign((size_t)F, 0);
    for (int f = 0; f < F; ++f) {
        int off = 0;
        for (int k = cl->first[(size_t)f]; k < cl->first[(size_t)f + 1]; ++k) { cl->off[(size_t)k] = off; off += cl->size[(size_t)k]; }
        cl->span[(size_t)f] = off;
        cl->points += off;
    }
    return ensure_clusters(c, cl->ncl, cl->points);
}

// d_koffx: the offsets the label scatter writes the ICP sources to, [copy][round][F][KICP].  Cluster q of frame f starts, in
// copy t, at off[q] + t * span[f] of the frame's segment.  copies == 1 is the table of the per-template passes; they pass
// nullptr (packed) for round 0, so its round-0 words are never read.
// Grows d_koffx (which synchronises the stream when it has to) and uploads the table with a blocking copy.
int upload_koffx(cd_context* c, int F, const BatchClusters& cl, int copies) {
    const size_t need = (size_t)copies * cl.rounds_k * F * KICP;
    GROW(c, d_koffx, need);
    std::vector<int> tab(need, 0);
    for (int t = 0; t < copies; ++t)
        for (int r = 0; r < cl.rounds_k; ++r)
            for (int f = 0; f < F; ++f)
                for (int k = 0; k < KICP; ++k) {
                    const int q = cl.first[(size_t)f] + r * KICP + k;
                    if (q < cl.first[(size_t)f + 1]) tab[(((size_t)t * cl.rounds_k + r) * F + f) * KICP + k] = cl.off[(size_t)q] + t * cl.span[(size_t)f];
                }
    HIPCHK(c, copy_sync(c, c->d_koffx, tab.data(), sizeof(int) * need, hipMemcpyHostToDevice));
    return CD_OK;
}
const int* koffx_at(const cd_context* c, int F, const BatchClusters& cl, int t, int r) { return c->d_koffx + (((size_t)t * cl.rounds_k + r) * F) * KICP; }

// Extraction round r of the ICP sources: the clusters ranked [r * KICP, (r + 1) * KICP) of every frame, to the offsets koff
// ([F][KICP]; nullptr: packed, round 0 only).  With a single round the tile counts of stage_cluster are still in d_tileK.
// Issues the label scatter, behind a memset, a count and a scan of d_tileK when there are several rounds; no synchronisation.
int extract_round(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, int r, const int* koff) {
    if (cl.rounds_k > 1) {
        HIPCHK(c, hipMemsetAsync(c->d_tileK, 0, sizeof(int) * (size_t)F * KICP * c->T, c->stream));
        LAUNCH(c, launch_label_count(c->stream, c->N, F, c->T, cl.To, c->d_fs, p->cluster_enable, c->d_parent, c->d_rank, c->d_label, c->d_tileK, r * KICP));
        LAUNCH(c, launch_scan_tiles(c->stream, c->d_tileK, F * KICP, c->T, nullptr, 0));
    }
    LAUNCH(c, launch_label_scatter(c->stream, c->d_obj, c->N, F, c->T, cl.To, c->d_fs, c->d_label, c->d_tileK, c->d_src0, c->d_src, r * KICP, koff));
    return CD_OK;
}

// (Re)builds the ICP sources d_src0 / d_src of every round (upload_koffx with one copy has run when there are several).
// Round 0 was extracted by stage_cluster; it is redone only when d_src has been consumed by a previous template pass or
// d_tileK by a later round.
int extract_sources(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, bool redo_round0) {
    for (int r = redo_round0 ? 0 : 1; r < cl.rounds_k; ++r)
        if (int e = extract_round(c, p, F, cl, r, r > 0 ? koffx_at(c, F, cl, 0, r) : nullptr)) return e;
    return CD_OK;
}

struct BatchIcp {   // the ICP part of a fused call; the results themselves are kept in c->last_clusters
    std::vector<int> slots;                    // the template slots every cluster is matched against, ascending
    std::vector<long long> orig_off, al_off;   // per cluster, see cd_get_cluster_points (publish_last hands them to the context)
    long long pairs = 0;                       // pair tests of all its stages
};

// The first statement of the ICP part: the per-cluster results of the previous batch go away.  last_first stays empty until
// publish_last, so a failure in between leaves cd_get_cluster_results with "no batch" rather than old offsets into new results.
// template_slot >= 0: every cluster against that slot; -1: against every loaded template.  Host only.
void begin_batch_icp(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    c->last_first.clear();
    if (p->template_slot >= 0) bi->slots.push_back(p->template_slot);
    else for (int sidx = 0; sidx < CD_MAX_TEMPLATES; ++sidx) if (c->tpl_m[sidx] > 0) bi->slots.push_back(sidx);
    if (bi->slots.empty()) bi->slots.push_back(0);
    c->last_clusters.assign((size_t)std::max(cl.ncl, 1), cd_cluster_result());
    bi->orig_off.assign((size_t)std::max(cl.ncl, 1), -1);
    bi->al_off.assign((size_t)std::max(cl.ncl, 1), -1);
    for (int f = 0; f < F; ++f)
        for (int q = cl.first[(size_t)f]; q < cl.first[(size_t)f + 1]; ++q) bi->orig_off[(size_t)q] = (long long)f * c->N + cl.off[(size_t)q];
}

// Several templates: when S copies of every frame's ICP sources fit its segment of the source buffers (they do unless a frame
// is nearly all objects), every (cluster, template) pair becomes one ICP problem of ONE stage - the batch then fills the chip
// with S x ncl problems instead of running S under-filled passes one after the other.
bool fits_one_stage(const cd_context* c, int F, const BatchClusters& cl, int S) {
    if (S <= 1 || cl.ncl <= 0 || (long long)S * cl.ncl > 0x3fffffffll) return false;
    for (int f = 0; f < F; ++f)
        if ((long long)S * cl.span[(size_t)f] > (long long)c->N) return false;
    return true;
}

// ICP problem q of the stage just run (synchronised by stage_icp) is cluster k against slots[t].  Its result is kept when it
// is the first (t == 0) or has the lower fitness, so ties keep the lowest slot.  `resident`: the problem's aligned points are
// still in d_src when the call returns (al_off; -1 otherwise).
void keep_lower_fitness(cd_context* c, const cd_params* p, BatchIcp* bi, int q, int k, int t, bool resident) {
    cd_cluster_result r;
    fill_cluster_result(c, q, p, &r);
    r.template_slot = bi->slots[(size_t)t];
    if (t > 0 && !(r.fitness < c->last_clusters[(size_t)k].fitness)) return;
    c->last_clusters[(size_t)k] = r;
    bi->al_off[(size_t)k] = resident ? (long long)c->h_cl[q].src_off : -1;
}

// CD_GUESS_CLUSTER: the records of the stage just run (h_shape, on the host since stage_icp's synchronisation) for
// cd_get_cluster_shape_frames - problem k < ncl is cluster k.
void keep_cluster_shapes(cd_context* c, const cd_params* p, int ncl) {
    if (p->icp_use_guess != CD_GUESS_CLUSTER) return;
    static_assert(sizeof(ShapeFrame) == sizeof(cd_shape_frame), "ShapeFrame mirrors cd_shape_frame");
    c->last_shapes.resize((size_t)ncl);
    if (ncl > 0) std::memcpy(c->last_shapes.data(), c->h_shape.get(), sizeof(ShapeFrame) * (size_t)ncl);
}

// All (cluster, template) pairs in one stage (fits_one_stage): problem t * ncl + k is cluster k against slots[t], on copy t of
// the sources.  Uploads the offset table of S copies, issues every extraction round of every copy and one stage_icp, which
// ends synchronised.  Every problem's aligned points stay resident.
int icp_all_pairs(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    const int S = (int)bi->slots.size(), ncl = cl.ncl;
    int st = upload_koffx(c, F, cl, S);
    if (st) return st;
    for (int t = 0; t < S; ++t)
        for (int r = 0; r < cl.rounds_k; ++r) {
            st = extract_round(c, p, F, cl, r, koffx_at(c, F, cl, t, r));
            if (st) return st;
        }
    st = ensure_clusters(c, S * ncl, (long long)S * cl.points);
    if (st) return st;
    for (int t = 0; t < S; ++t)
        for (int f = 0; f < F; ++f) {
            const int q = cl.first[(size_t)f];
            set_icp_clusters(c, t * ncl + q, c->h_fs[f].n_k, f, cl.size.data() + q, cl.off.data() + q, f * c->N + t * cl.span[(size_t)f], bi->slots[(size_t)t]);
        }
    st = stage_icp(c, S * ncl, p, &bi->pairs);
    if (st) return st;
    keep_cluster_shapes(c, p, ncl);   // (the problems of slots[0]: a cluster's record does not depend on the template)
    for (int t = 0; t < S; ++t)
        for (int k = 0; k < ncl; ++k) keep_lower_fitness(c, p, bi, t * ncl + k, k, t, true);
    return CD_OK;
}

// One ICP pass per slot, every cluster against it.  The sources are re-extracted between passes (ICP transforms d_src in
// place), so the aligned cloud of a pass stays in d_src only until the next one: only the last slot's is resident.
// Uploads the later rounds' offsets when there are several rounds; per pass: extract_sources, then one stage_icp, which ends
// synchronised.
int icp_per_template(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    const int S = (int)bi->slots.size();
    if (cl.rounds_k > 1)
        if (int e = upload_koffx(c, F, cl, 1)) return e;
    for (int t = 0; t < S; ++t) {
        int st = extract_sources(c, p, F, cl, t > 0);
        if (st) return st;
        for (int f = 0; f < F; ++f) {
            const int q = cl.first[(size_t)f];
            set_icp_clusters(c, q, c->h_fs[f].n_k, f, cl.size.data() + q, cl.off.data() + q, f * c->N, bi->slots[(size_t)t]);
        }
        long long pr = 0;
        st = stage_icp(c, cl.ncl, p, &pr);
        if (st) return st;
        keep_cluster_shapes(c, p, cl.ncl);
        bi->pairs += pr;
        for (int k = 0; k < cl.ncl; ++k) keep_lower_fitness(c, p, bi, k, k, t, t + 1 == S);
    }
    return CD_OK;
}

// The state behind the read-back calls (cd_get_cluster_results, cd_get_cluster_points, cd_get_frame_cloud), published once
// every ICP stage of the batch has succeeded: the only place last_first is assigned.  Host only.
void publish_last(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    c->last_first = cl.first;
    c->last_orig_off.swap(bi->orig_off);
    c->last_al_off.swap(bi->al_off);
    c->last_nv.resize((size_t)F); c->last_no.resize((size_t)F);
    for (int f = 0; f < F; ++f) { c->last_nv[(size_t)f] = c->h_fs[f].n_v; c->last_no[(size_t)f] = c->h_fs[f].n_o; }
    c->last_clouds = true;
    c->last_surface_ok = p->icp_use_guess == CD_GUESS_SURFACE;
    c->last_shapes_ok = p->icp_use_guess == CD_GUESS_CLUSTER;
    if (c->last_shapes_ok && cl.ncl == 0) c->last_shapes.clear();
}

// The per-frame records from h_fs, the plane mirrors and c->last_clusters, and the byte counts of the timing
// (algorithmic_bytes, icp_algorithmic_bytes).  Host only; every stage has been synchronised.
void write_frame_records(cd_context* c, int N, int F, const BatchClusters& cl, const FrontStages& fr, cd_frame_result* results) {
    static_assert(offsetof(ShapeFrame, mean) == offsetof(cd_shape_frame, mean) && offsetof(ShapeFrame, hi) == offsetof(cd_shape_frame, hi), "ShapeFrame mirrors cd_shape_frame");
    long long balg = 0;
    for (int f = 0; f < F; ++f) {
        const FrameState& s = c->h_fs[f];
        cd_frame_result& r = results[f];
        std::memset(&r, 0, sizeof(r));
        r.status = s.status;
        r.n_cropped = s.n_cropped;
        r.n_voxels = s.n_v;
        r.n_plane = s.n_plane;
        r.n_objects = s.n_o;
        r.n_clusters = s.n_k;
        r.flags = s.n_k > KICP ? CD_FRAME_MORE_CLUSTERS : 0;
        if (!fr.surface_flag.empty() && fr.surface_flag[(size_t)f]) r.flags |= CD_FRAME_SURFACE_GUESS;
        r.ransac_iterations = fr.iterations[f];
        if (s.status == CD_OK && !c->h_have[f]) r.status = CD_ERR_NO_MODEL;
        if (c->h_have[f]) { r.plane[0] = c->h_model[f].x; r.plane[1] = c->h_model[f].y; r.plane[2] = c->h_model[f].z; r.plane[3] = c->h_model[f].w; }
        balg += 12ll * N + 12ll * s.n_v + 12ll * s.n_v * (fr.rounds + 3) + 4ll * s.n_v + 16ll * s.n_o + 200ll * s.n_k;
        for (int k = 0; k < s.n_k; ++k) {
            const cd_cluster_result& cr = c->last_clusters[(size_t)(cl.first[(size_t)f] + k)];
            if (k < KICP) r.clusters[k] = cr;
            if (c->last_shapes_ok) {   // CD_GUESS_CLUSTER: did this cluster's ICP (against the template it kept) start from a rule-C13 guess?
                ShapeFrame rec;
                float G[16];
                std::memcpy(&rec, &c->last_shapes[(size_t)(cl.first[(size_t)f] + k)], sizeof(rec));
                if (shape_guess(rec, template_frame(c, cr.template_slot), G) >= 0) r.flags |= CD_FRAME_CLUSTER_GUESS;
            }
            const long long b = 12ll * c->tpl_m[cr.template_slot] + 12ll * cr.size * (cr.iterations + 1);
            balg += b;
            c->timing.icp_algorithmic_bytes += b;
        }
    }
    c->timing.algorithmic_bytes = balg;
}

// The optional plane_inliers / labels outputs ([F][N], -1 beyond a frame's count): one blocking D2H copy per frame and output.
int copy_frame_indices(cd_context* c, int N, int F, int32_t* plane_inliers, int32_t* labels) {
    for (int f = 0; f < F && (plane_inliers || labels); ++f) {
        const FrameState& s = c->h_fs[f];
        if (plane_inliers) {
            int32_t* dst = plane_inliers + (size_t)f * N;
            std::fill(dst, dst + N, -1);
            if (s.n_plane > 0) HIPCHK(c, copy_sync(c, dst, c->d_plane_idx + (size_t)f * c->N, sizeof(int) * s.n_plane, hipMemcpyDeviceToHost));
        }
        if (labels) {
            int32_t* dst = labels + (size_t)f * N;
            std::fill(dst, dst + N, -1);
            if (s.n_o > 0) HIPCHK(c, copy_sync(c, dst, c->d_label + (size_t)f * c->N, sizeof(int) * s.n_o, hipMemcpyDeviceToHost));
        }
    }
    return CD_OK;
}

// The stage times between the events ev[0..4] of process_batch_impl ([4]: the whole call) and the pair-test count.
// Waits for ev[4].
int read_stage_timing(cd_context* c, long long pairs) {
    HIPCHK(c, hipEventSynchronize(c->ev[4]));
    for (int k = 0; k < 4; ++k) hipEventElapsedTime(&c->timing.stage_ms[k], c->ev[k], c->ev[k + 1]);
    hipEventElapsedTime(&c->timing.stage_ms[4], c->ev[0], c->ev[4]);
    c->timing.icp_pair_tests_lo = (int32_t)(pairs & 0xffffffffll);
    c->timing.icp_pair_tests_hi = (int32_t)(pairs >> 32);
    return CD_OK;
}

// cd_get_frame_bboxes: the rectangles this call's gate used.  Host only; the colour records' mirrors (h_crec, h_cstatus) have
// been valid since the call's first synchronisation.
int publish_bboxes(cd_context* c, int gate_source, int F) {
    if (gate_source == CD_BBOX_PARAMS) return CD_OK;
    c->last_bboxes.assign((size_t)F, cd_color_bbox{});
    for (int f = 0; f < F; ++f) {
        if (gate_source == CD_BBOX_COLOR) std::memcpy(&c->last_bboxes[(size_t)f], &c->h_crec[f], sizeof(cd_color_bbox));
        else { std::memcpy(c->last_bboxes[(size_t)f].rect, c->frame_rects.data() + 4 * (size_t)f, sizeof(int32_t) * 4); c->last_bboxes[(size_t)f].found = 1; }
    }
    if (gate_source == CD_BBOX_COLOR)
        if (int st = color_status(c, F)) return st;
    c->last_bboxes_ok = true;
    return CD_OK;
}

// The fused call, in the order of DESIGN.md §5.  The event records ev[0..4] (the boundaries of cd_timing.stage_ms) and the
// release of the front gate are all here.
int process_batch_impl(cd_context* c, const void* d_frames, size_t stride, int N, int F, const cd_params* p,
                       cd_frame_result* results, int32_t* plane_inliers, int32_t* labels, const DepthJob* dj = nullptr) {
    // checks: nothing is copied or launched before they have passed
    int st = check_params(c, p);
    if (!st) st = check_bbox_source(c, p, F, dj && dj->color);
    if (st) return st;
    if (!results || !d_frames) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (N <= 0 || F <= 0 || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad shape/stride");
    if (N > c->N || F > c->F) return fail(c, CD_ERR_CAPACITY, "batch larger than the context capacity");
    invalidate_last(c);
    std::memset(&c->timing, 0, sizeof(c->timing));
    BatchGuard in_flight(c->device);
    GateHold front;
    if (c->front_concurrent > 0) front.enter(&g_front_gate[c->device & (MAX_DEVICES - 1)], c->front_concurrent);
    const int gate_source = p->bbox_enable ? c->bbox_source : CD_BBOX_PARAMS;
    BatchScope scope{c};
    // [0] gate rectangles, deprojection, zero launch, crop + voxel grid
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    st = batch_prologue(c, gate_source, d_frames, F, dj);
    if (!st) st = stage_crop_voxel(c, d_frames, stride, N, F, p, nullptr);
    if (!st) st = sync_fs(c, F);   // n_v
    if (st) return st;
    // [1] plane
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    FrontStages fr;
    st = stage_plane(c, F, p, fr.iterations, &fr.rounds);
    if (st) return st;
    // [2] extract, cluster, surface guesses
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    st = stage_extract(c, F, p);
    if (!st) st = sync_fs(c, F, c->mirror_writes && c->copy_kernels);   // n_o per frame (written to the mirror by the scan): picks the clustering path and sizes the launches
    if (st) return st;
    int max_no = 0;
    for (int f = 0; f < F; ++f) max_no = std::max(max_no, c->h_fs[f].n_o);
    st = stage_cluster_sync(c, F, p, max_no);   // sync #4: n_plane, n_o, n_k, ksize, koff
    if (!st && p->icp_use_guess == CD_GUESS_SURFACE) st = surface_guesses(c, F, p, &fr.surface_flag);
    if (st) return st;
    // [3] ICP of every cluster, against one template or all of them
    HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    front.release();
    BatchClusters cl;
    st = batch_clusters(c, F, &cl);
    if (st) return st;
    BatchIcp bi;
    begin_batch_icp(c, p, F, cl, &bi);
    if (fits_one_stage(c, F, cl, (int)bi.slots.size())) st = icp_all_pairs(c, p, F, cl, &bi);
    else st = icp_per_template(c, p, F, cl, &bi);
    if (st) return st;
    publish_last(c, p, F, cl, &bi);
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    // records and read-out
    write_frame_records(c, N, F, cl, fr, results);
    st = copy_frame_indices(c, N, F, plane_inliers, labels);
    if (!st) st = read_stage_timing(c, bi.pairs);
    if (!st) st = publish_bboxes(c, gate_source, F);
    return st;
}

}  // namespace

// ==========================================================================================
extern "C" {

void cd_default_params(cd_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->crop_z_min = 0.0; p->crop_z_max = 0.9;            // gps.cpp:56
    p->crop_x_min = -0.2; p->crop_x_max = 0.2;           // gps.cpp:64
    p->leaf_size = 0.005f;                               // ground_plane_segmentation.launch:16
    p->rgb_offset = -1;
    p->plane_distance_threshold = 0.015;                 // ground_plane_segmentation.launch:18
    p->plane_max_iterations = 1000;                      // gps.cpp:88
    p->plane_optimize = 1;                               // gps.cpp:85
    p->plane_probability = 0.99;                         // PCL default
    p->extract_negative = 1;                             // launch: invert: true
    p->crop2_enable = 1; p->crop2_z_min = 0.0; p->crop2_z_max = 0.75;   // opd.cpp:335
    p->cluster_enable = 1;
    p->cluster_min_size = 200; p->cluster_max_size = 25000;             // opd.cpp:357-358
    p->cluster_tolerance = 0.02;                         // opd.cpp:356
    p->icp_max_iterations = 5000;                        // icp.cpp:173
    p->template_slot = 0;
    p->plane_model = CD_PLANE;
    p->plane_eps_angle = 0.0;
    p->icp_transformation_epsilon = 1e-9;                // icp.cpp:174
    p->icp_euclidean_fitness_epsilon = 0.0004;           // icp.cpp:176 + launch:42
    p->icp_accept_fitness = 0.0004;                      // icp.cpp:182
}

int cd_abi_version(void) { return CD_ABI_VERSION; }

int cd_struct_size(int which) {
    switch (which) {
        case 0: return (int)sizeof(cd_params);
        case 1: return (int)sizeof(cd_cluster_result);
        case 2: return (int)sizeof(cd_frame_result);
        case 3: return (int)sizeof(cd_timing);
        case 4: return (int)sizeof(cd_depth_camera);
        case 5: return (int)sizeof(cd_color_gate_params);
        case 6: return (int)sizeof(cd_color_bbox);
        case 7: return (int)sizeof(cd_overlay_params);
        case 8: return (int)sizeof(cd_overlay_box);
        default: return -1;
    }
}

const char* cd_last_error(const cd_context* ctx) { return ctx ? ctx->err : "null context"; }

void cd_destroy(cd_context* c) {
    if (!c) return;
    hipSetDevice(c->device);
    for (hipStream_t q : {c->stream, c->stream2, c->stream3}) if (q) hipStreamSynchronize(q);
    // the members free their memory, then ~cd_streams destroys the events and the (drained) streams
    delete c;
}

int cd_create(int device_id, int max_points, int max_frames, cd_context** out) {
    if (!out) return CD_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_points <= 0 || max_frames <= 0) return CD_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return CD_ERR_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return CD_ERR_DEVICE;
    cd_context* c = new cd_context();
#define ALLOC(buf, n) (c->buf.alloc((n), #buf) == hipSuccess)
    c->device = device_id;
    c->N = max_points;
    c->F = max_frames;
    c->T = (max_points + TILE - 1) / TILE;
    const size_t N = (size_t)c->N, F = (size_t)c->F, T = (size_t)c->T, FN = F * N;
    // non-blocking: no implicit ordering against the NULL stream (torch ops, other contexts in flight)
    if (const char* m = std::getenv("CUBOID_ICP_LOWPRIO")) c->icp_lowprio = std::atoi(m);
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_least = prio_greatest = 0;
    bool ok = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, 0) == hipSuccess;
    for (auto& e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && ALLOC(d_fs, F) && ALLOC(h_fs, F);
    ok = ok && ALLOC(d_tileA, F * T) && ALLOC(d_tileB, F * T) && ALLOC(d_tileK, F * KICP * T) && ALLOC(d_tileC, F * T);
    ok = ok && ALLOC(d_cpt, FN) && ALLOC(d_vox, FN) && ALLOC(d_obj, FN);
    ok = ok && ALLOC(d_src0, FN) && ALLOC(d_src, FN);
    for (int k = 0; k < 2; ++k) ok = ok && ALLOC(d_key[k], FN) && ALLOC(d_val[k], FN);
    ok = ok && ALLOC(d_ghist, F * SORT_MAX_PASSES_HOST * RADIX);
    ok = ok && ALLOC(d_sstate, (size_t)SORT_MAX_PASSES_HOST * F * RADIX * ((N + SCATTER_TILE - 1) / SCATTER_TILE));   // (per scatter tile: run and point counts are at most N)
    ok = ok && ALLOC(d_tile64, F * T);
    ok = ok && ALLOC(d_ticket, (size_t)F * TICKET_PITCH) && hipMemset(c->d_ticket, 0, sizeof(int) * (size_t)F * TICKET_PITCH) == hipSuccess;
    ok = ok && ALLOC(d_rnd, (size_t)RND_TABLE);
    ok = ok && ALLOC(d_models, F * MAX_HYP) && ALLOC(d_valid, F * MAX_HYP) && ALLOC(d_counts, F * MAX_HYP);
    ok = ok && ALLOC(h_valid, F * MAX_HYP) && ALLOC(h_counts, F * MAX_HYP) && ALLOC(h_models, F * MAX_HYP);
    ok = ok && ALLOC(d_active, F) && ALLOC(h_active, F);
    ok = ok && ALLOC(d_model, F) && ALLOC(h_model, F);
    ok = ok && ALLOC(d_have, F) && ALLOC(h_have, F);
    ok = ok && ALLOC(d_sums, F * 10) && ALLOC(h_sums, F * 10);
    ok = ok && ALLOC(d_plane_idx, FN) && ALLOC(d_head, F * CELL_BUCKETS);
    ok = ok && ALLOC(d_next, FN) && ALLOC(d_parent, FN) && ALLOC(d_csize, FN);
    ok = ok && ALLOC(d_rank, FN) && ALLOC(d_cand, FN) && ALLOC(d_sizes, FN) && ALLOC(d_label, FN);
    c->tpl_cap = 1 << 18;
    ok = ok && ALLOC(d_tpl, (size_t)c->tpl_cap);
    ok = ok && ALLOC(d_super, (size_t)CD_MAX_TEMPLATES);
    ok = ok && ALLOC(d_lat, (size_t)CD_MAX_TEMPLATES);
    {
        const int prio = c->icp_lowprio ? prio_least : 0;
        ok = ok && hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio) == hipSuccess;
        ok = ok && hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, prio) == hipSuccess;
    }
    for (auto& e : c->ev2) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    ok = ok && ALLOC(d_grid, (size_t)CD_MAX_TEMPLATES) && ALLOC(d_tcell, (size_t)CD_MAX_TEMPLATES * ICP_CELL_STRIDE);
    ok = ok && ALLOC(d_tlo, (size_t)c->tpl_cap / ICP_SUB) && ALLOC(d_thi, (size_t)c->tpl_cap / ICP_SUB);
    ok = ok && ALLOC(d_kdmap, (size_t)c->tpl_cap);
    ok = ok && ALLOC(d_tplk, (size_t)c->tpl_cap) && ALLOC(d_tlok, (size_t)c->tpl_cap / ICP_SUB) && ALLOC(d_thik, (size_t)c->tpl_cap / ICP_SUB);
    ok = ok && ALLOC(d_nn, FN) && ALLOC(d_d2, FN) && ALLOC(d_queue, (size_t)16) && ALLOC(d_don, (size_t)(DON_BOX + DON_CAP)) && ALLOC(d_wgtab, (size_t)3 * 1024);
    ok = ok && ALLOC(h_wgtab, (size_t)3 * 1024) && ALLOC(h_ctl, (size_t)16);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    }
    const size_t ncl = F * KICP;
    c->cl_cap = (int)ncl;
    c->work_cap = (int)(F * (N / 64 + KICP + 1));
    ok = ok && ALLOC(d_cl, ncl) && ALLOC(h_cl, ncl);
    ok = ok && ALLOC(d_order, ncl) && ALLOC(h_order, ncl);
    if (const char* m = std::getenv("CUBOID_ICP_MAX_WG")) c->icp_max_wg = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_ICP_CPW")) c->icp_cpw = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_ICP_SLOTS")) c->icp_slots = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_ICP_DONATE")) c->icp_donate = std::atoi(m);
    if (const char* m = std::getenv("CUBOID_ICP_DON_IDLE")) c->don_idle = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_ICP_DON_FAULT")) c->don_fault = std::atoi(m);
    if (const char* m = std::getenv("CUBOID_ICP_LATTICE")) c->icp_lattice = std::atoi(m);
    if (const char* m = std::getenv("CUBOID_COPY_KERNELS")) c->copy_kernels = std::atoi(m);
    if (const char* m = std::getenv("CUBOID_ZERO_ONCE")) c->zero_once = std::atoi(m);
    if (const char* m = std::getenv("CUBOID_LAT_SHAPE")) std::sscanf(m, "%d,%d,%d", &c->lat_shape[0], &c->lat_shape[1], &c->lat_shape[2]);
    if (const char* m = std::getenv("CUBOID_VOXEL_RUNS")) c->voxel_runs = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_CENTROID_LANES")) c->centroid_lanes = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_CROP_DIRECT")) c->crop_direct = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_CLUSTER_CELLS")) c->cluster_cells = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_MIRROR_WRITES")) c->mirror_writes = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_MIRROR_READS")) c->mirror_reads = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_ICP_DIRECT")) c->icp_direct = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_ICP_BIG_WEIGHT")) c->icp_big_weight = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_CROP_TWO_PASS")) c->crop_two_pass = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_ICP_PERSIST")) c->icp_persist = std::atoi(m);
    if (const char* m = std::getenv("CUBOID_FORCE_SCAN_STALL")) c->force_stall = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_CROP_RUNS")) c->crop_runs = std::atoi(m) != 0;
    if (const char* m = std::getenv("CUBOID_ICP_CONCURRENT")) c->icp_concurrent = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_FRONT_CONCURRENT")) c->front_concurrent = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("CUBOID_ICP_MODE")) c->icp_mode = !std::strcmp(m, "sliced") ? 1 : (!std::strcmp(m, "cluster") ? 2 : (!std::strcmp(m, "pipe") ? 3 : 0));
    ok = ok && ALLOC(d_work, (size_t)c->work_cap) && ALLOC(h_work, (size_t)c->work_cap);
    ok = ok && ALLOC(d_work2, (size_t)c->work_cap) && ALLOC(h_work2, (size_t)c->work_cap);
    ok = ok && ALLOC(d_st, ncl * 2) && ALLOC(h_st, ncl * 2);
    ok = ok && ALLOC(d_acc, ncl * 48) && ALLOC(d_accf, ncl + 1) && ALLOC(h_accf, ncl + 1);
    ok = ok && ALLOC(d_ctab, (size_t)512) && ALLOC(d_crec, F) && ALLOC(h_crec, F);
    ok = ok && ALLOC(d_cstatus, F) && ALLOC(h_cstatus, F);
    ok = ok && ALLOC(d_rects, F * 4) && ALLOC(h_rects, F * 4);
    cd_default_color_gate_params(&c->color_prm);
    if (ok) {   // rule C10 step 1: sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)), in double, half to even
        std::vector<int> tab(512, 0);
        for (int i = 1; i < 256; ++i) {
            tab[(size_t)i] = (int)std::nearbyint((double)(255 << 12) / (double)i);
            tab[256 + (size_t)i] = (int)std::nearbyint((double)(180 << 12) / (6.0 * (double)i));
        }
        ok = copy_sync(c, c->d_ctab, tab.data(), sizeof(int) * 512, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        // PCL's SAC sampler: boost::mt19937 seeded 12345, uniform_int<>(0, INT_MAX) == mt() >> 1
        std::vector<int> tab((size_t)RND_TABLE);
        std::mt19937 gen(12345u);
        for (auto& v : tab) v = (int)(gen() >> 1);
        ok = copy_sync(c, c->d_rnd, tab.data(), sizeof(int) * RND_TABLE, hipMemcpyHostToDevice) == hipSuccess;
    }
#undef ALLOC
    if (!ok) {
        cd_destroy(c);
        return CD_ERR_DEVICE;
    }
    *out = c;
    return CD_OK;
}

// ---- templates ------------------------------------------------------------------------------------------------------
// Everything cd_set_template derives from the template's points is device-independent host work (template_prep.hpp): it is
// done once per distinct template and shared by every context of the process (bench.py keeps three contexts per GPU; the
// reference re-reads and re-indexes the template for every frame, icp.cpp:159).  The cache is process-wide, keyed on m plus the
// raw bytes, and keeps the 16 newest entries.
// (cell_factor is tuning only and not part of the key: a cached template keeps the factor it was prepared with)
static std::shared_ptr<const PreparedTemplate> prepared_template_cached(const void* xyz, size_t stride, int m, float cell_factor) {
    const std::vector<float> raw = gather_xyz(xyz, stride, m);
    static std::mutex mu;
    static std::vector<std::shared_ptr<const PreparedTemplate>> cache;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const auto& e : cache)
            if (e->m == m && std::memcmp(e->xyz.data(), raw.data(), raw.size() * sizeof(float)) == 0) return e;
    }
    std::shared_ptr<const PreparedTemplate> P = prepare_template(raw.data(), m, cell_factor);
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() >= 16) cache.erase(cache.begin());
    cache.push_back(P);
    return P;
}

// copies a prepared template into the context's template arena at point offset `off` (a multiple of 64)
static int upload_template(cd_context* c, int slot, int off, const PreparedTemplate& P) {
    const int nrun = P.m_pad / ICP_SUB;
    HIPCHK(c, copy_sync(c, c->d_tpl + off, P.cell_pts.data(), sizeof(float4) * (size_t)P.m_pad, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_tlo + off / ICP_SUB, P.cell_lo.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_thi + off / ICP_SUB, P.cell_hi.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_tplk + off, P.kd_pts.data(), sizeof(float4) * (size_t)P.m_pad, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_tlok + off / ICP_SUB, P.kd_lo.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_thik + off / ICP_SUB, P.kd_hi.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    if (!P.kdmap.empty())
        HIPCHK(c, copy_sync(c, c->d_kdmap + off, P.kdmap.data(), sizeof(unsigned short) * P.kdmap.size(), hipMemcpyHostToDevice));
    IcpGrid grid = P.grid;
    grid.cell_off = slot * ICP_CELL_STRIDE;
    if (!P.cell_start.empty())
        HIPCHK(c, copy_sync(c, c->d_tcell + grid.cell_off, P.cell_start.data(), sizeof(unsigned short) * P.cell_start.size(), hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_grid + slot, &grid, sizeof(grid), hipMemcpyHostToDevice));
    c->tpl_off[slot] = off;
    c->tpl_m[slot] = P.m;
    c->tpl_gridded[slot] = grid.ncell > 0;
    c->tpl_big[slot] = P.big_ok;
    HIPCHK(c, copy_sync(c, c->d_super + slot, &P.super, sizeof(IcpSuper), hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_lat + slot, &P.lat, sizeof(IcpLattice), hipMemcpyHostToDevice));
    c->tpl_faces[slot] = P.lat.nface;
    c->tpl_frame[slot] = P.frame;
    c->tframe_dirty = true;   // (rule C13's slot table: uploaded by the next CD_GUESS_CLUSTER stage)
    return CD_OK;
}

int cd_set_template(cd_context* c, int slot, const void* xyz, size_t stride, int m) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (slot < 0 || slot >= CD_MAX_TEMPLATES || !xyz || m <= 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad template arguments");
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float cell_factor = 2.0f;
    if (const char* e = std::getenv("CUBOID_ICP_CELL_FACTOR")) cell_factor = (float)std::atof(e);   // tuning only
    std::shared_ptr<const PreparedTemplate> P = prepared_template_cached(xyz, stride, m, cell_factor);
    // a slot is re-used in place when the new template fits its space, appended otherwise; when the arena is full the
    // live slots are packed again (the space of replaced templates is reclaimed) before giving up
    const int old_pad = c->tpl_prep[slot] ? c->tpl_prep[slot]->m_pad : 0;
    if (old_pad >= P->m_pad) {
        c->tpl_prep[slot] = P;
        return upload_template(c, slot, c->tpl_off[slot], *P);
    }
    if (c->tpl_used + P->m_pad <= c->tpl_cap) {
        const int off = c->tpl_used;
        c->tpl_used += P->m_pad;
        c->tpl_prep[slot] = P;
        return upload_template(c, slot, off, *P);
    }
    long long total = P->m_pad;
    for (int k = 0; k < CD_MAX_TEMPLATES; ++k) if (k != slot && c->tpl_prep[k]) total += c->tpl_prep[k]->m_pad;
    if (total > c->tpl_cap) return fail(c, CD_ERR_CAPACITY, "template storage exhausted");
    c->tpl_prep[slot] = P;
    int off = 0;
    for (int k = 0; k < CD_MAX_TEMPLATES; ++k) {
        if (!c->tpl_prep[k]) continue;
        if (int ust = upload_template(c, k, off, *c->tpl_prep[k])) return ust;
        off += c->tpl_prep[k]->m_pad;
    }
    c->tpl_used = off;
    return CD_OK;
}

int cd_template_lattice_faces(const cd_context* c, int slot) {
    if (!c || slot < 0 || slot >= CD_MAX_TEMPLATES) return CD_ERR_INVALID_ARG;
    if (c->tpl_m[slot] <= 0) return CD_ERR_NO_TEMPLATE;
    return c->tpl_faces[slot];
}

int cd_lattice_detect(const void* xyz, size_t stride, int m, int32_t* out) {
    if (!xyz || m <= 0 || stride < 12) return CD_ERR_INVALID_ARG;
    const std::vector<float> raw = gather_xyz(xyz, stride, m);
    auto L = std::make_unique<IcpLattice>();
    lattice_detect(raw.data(), m, L.get());
    for (int f = 0; out && f < L->nface; ++f) {
        const int w = L->w[f], u = L->fast[f], v = 3 - w - u;
        const int32_t row[5] = {w, u, L->base[f], L->n[u], L->n[v]};
        std::memcpy(out + 5 * f, row, sizeof(row));
    }
    return L->nface;
}

int cd_lattice_axes(const void* xyz, size_t stride, int m, int32_t* out_axis_face, float* out_axis_c) {
    if (!xyz || m <= 0 || stride < 12) return CD_ERR_INVALID_ARG;
    const std::vector<float> raw = gather_xyz(xyz, stride, m);
    auto L = std::make_unique<IcpLattice>();
    lattice_detect(raw.data(), m, L.get());
    if (L->nface == 0) lattice_classify_axes(L.get());   // (not a lattice: the "none" values)
    if (out_axis_face) std::memcpy(out_axis_face, L->axis_face, sizeof(L->axis_face));
    if (out_axis_c) std::memcpy(out_axis_c, L->axis_c, sizeof(L->axis_c));
    return L->axes_distinct;
}

int cd_template_nearest(cd_context* c, int slot, const void* queries, size_t stride, int n, int32_t* out_index, float* out_d2) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (slot < 0 || slot >= CD_MAX_TEMPLATES || !queries || n <= 0 || stride < 12 || !out_index || !out_d2) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (c->tpl_m[slot] <= 0) return fail(c, CD_ERR_NO_TEMPLATE, "template slot empty");
    if (c->tpl_faces[slot] <= 0) return fail(c, CD_ERR_INVALID_ARG, "the slot's template is not a lattice: its nearest-neighbour searches only exist inside the ICP kernels");
    if ((long long)n > (long long)c->N * c->F) return fail(c, CD_ERR_CAPACITY, "more queries than the context holds points");
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = upload_points(c, queries, stride, n, c->d_src0);
    if (st) return st;
    LAUNCH(c, launch_lat_nn(c->stream, c->d_lat + slot, c->d_src0, n, c->d_nn, c->d_d2));
    HIPCHK(c, copy_sync(c, out_index, c->d_nn, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, out_d2, c->d_d2, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return CD_OK;
}

static int cd_crop_voxel_impl(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float* out_xyz,
                  uint32_t* out_rgb, int capacity, int* out_n_cropped, int* out_n_voxels) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!points || !out_xyz || n < 0 || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (out_n_cropped) *out_n_cropped = 0;
    if (out_n_voxels) *out_n_voxels = 0;
    if (n == 0) return CD_OK;
    st = ensure_input(c, (size_t)n * stride);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, (size_t)n * stride, hipMemcpyHostToDevice, c->stream));
    st = stage_crop_voxel(c, c->d_in, stride, n, 1, p, nullptr);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const FrameState& s = c->h_fs[0];
    if (out_n_cropped) *out_n_cropped = s.n_cropped;
    if (s.status != CD_OK) return fail(c, s.status, "voxel grid: leaf size too small for the input extent");
    if (s.n_v > capacity) return fail(c, CD_ERR_CAPACITY, "output capacity too small");
    std::vector<float4> tmp((size_t)std::max(s.n_v, 1));
    HIPCHK(c, copy_sync(c, tmp.data(), c->d_vox, sizeof(float4) * s.n_v, hipMemcpyDeviceToHost));
    for (int i = 0; i < s.n_v; ++i) {
        out_xyz[3 * i] = tmp[i].x; out_xyz[3 * i + 1] = tmp[i].y; out_xyz[3 * i + 2] = tmp[i].z;
        if (out_rgb) std::memcpy(&out_rgb[i], &tmp[i].w, 4);
    }
    if (out_n_voxels) *out_n_voxels = s.n_v;
    return CD_OK;
}

// helper: load a caller cloud as the (single-frame) voxel cloud / object cloud
static int load_as(cd_context* c, const void* xyz, size_t stride, int n, float4* dst, int32_t FrameState::*count) {
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    int st = upload_points(c, xyz, stride, n, dst);
    if (st) return st;
    std::memset(&c->h_fs[0], 0, sizeof(FrameState));
    c->h_fs[0].*count = n;
    // origin for the cluster hash: min of the cloud
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    const char* b = (const char*)xyz;
    for (int i = 0; i < n; ++i) {
        float v[3];
        std::memcpy(v, b + (size_t)i * stride, 12);
        for (int a = 0; a < 3; ++a) if (v[a] < mn[a]) mn[a] = v[a];
    }
    for (int a = 0; a < 3; ++a) c->h_fs[0].origin[a] = n > 0 ? mn[a] : 0.f;
    HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
    return CD_OK;
}

static int cd_segment_plane_impl(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, float coeff[4],
                     int32_t* inliers, int capacity, int* out_n_inliers, int* out_iterations) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!xyz || !coeff || !inliers || n < 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (out_n_inliers) *out_n_inliers = 0;
    if (out_iterations) *out_iterations = 0;
    st = load_as(c, xyz, stride, n, c->d_vox, &FrameState::n_v);
    if (st) return st;
    std::vector<int> iters;
    st = stage_plane(c, 1, p, iters, nullptr);
    if (st) return st;
    if (out_iterations) *out_iterations = iters[0];
    if (!c->h_have[0]) return CD_ERR_NO_MODEL;
    cd_params q = *p;
    q.extract_negative = 1;
    q.crop2_enable = 0;
    st = stage_extract(c, 1, &q);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const int ni = c->h_fs[0].n_plane;
    if (ni > capacity) return fail(c, CD_ERR_CAPACITY, "inlier capacity too small");
    if (ni > 0) HIPCHK(c, copy_sync(c, inliers, c->d_plane_idx, sizeof(int) * ni, hipMemcpyDeviceToHost));
    coeff[0] = c->h_model[0].x; coeff[1] = c->h_model[0].y; coeff[2] = c->h_model[0].z; coeff[3] = c->h_model[0].w;
    if (out_n_inliers) *out_n_inliers = ni;
    return CD_OK;
}

// surface_normal_estimation.cpp:167-234.  The three constrained fits run on the device (cd_segment_plane's
// stages); the bookkeeping between them (ExtractIndices, pcl::compute3DCentroid - a sequential float32 sum -,
// the size sort, the handedness flip and the pose assembly) is the callback's own host code.
static int cd_surface_frame_impl(cd_context* c, const void* xyz, size_t stride, int n, const float table_normal[3], int invert,
                     const cd_params* p, cd_surface_frame_result* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if ((!xyz && n > 0) || !table_normal || !out || n < 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    std::memset(out, 0, sizeof(*out));
    struct P3 { float x, y, z; };
    std::vector<P3> cloud((size_t)n);
    for (int i = 0; i < n; ++i) std::memcpy(&cloud[(size_t)i], (const char*)xyz + (size_t)i * stride, 12);
    float normals[3][4], mids[3][4];
    int counts[3];
    for (int i = 0; i < 3; ++i) {   // sne.cpp:183-197
        cd_params q = *p;
        q.plane_model = i == 0 ? CD_PLANE_PERPENDICULAR : CD_PLANE_PARALLEL;
        for (int a = 0; a < 3; ++a) q.plane_axis[a] = table_normal[a];
        q.plane_eps_angle = 0.1;                       // sne.cpp:123
        q.plane_optimize = 1;                          // sne.cpp:118
        q.plane_max_iterations = 1000;                 // sne.cpp:125
        q.extract_negative = 1;
        q.crop2_enable = 0;
        q.bbox_enable = 0;
        const int m = (int)cloud.size();
        if (m > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
        st = load_as(c, cloud.data(), sizeof(P3), m, c->d_vox, &FrameState::n_v);
        if (st) return st;
        std::vector<int> iters;
        st = stage_plane(c, 1, &q, iters, nullptr);
        if (st) return st;
        out->iterations[i] = iters[0];
        if (!c->h_have[0]) return CD_ERR_NO_MODEL;
        st = stage_extract(c, 1, &q);
        if (st) return st;
        st = sync_fs(c, 1);
        if (st) return st;
        const int ni = c->h_fs[0].n_plane;
        std::vector<int> inl((size_t)std::max(ni, 1));
        if (ni > 0) HIPCHK(c, copy_sync(c, inl.data(), c->d_plane_idx, sizeof(int) * ni, hipMemcpyDeviceToHost));
        // getNormal(): plane_pc = ExtractIndices(negative = !invert), leftover = ExtractIndices(negative = invert)
        std::vector<char> is_inl((size_t)std::max(m, 1), 0);
        for (int k = 0; k < ni; ++k) is_inl[(size_t)inl[(size_t)k]] = 1;
        std::vector<P3> plane_pc, leftover;
        for (int k = 0; k < m; ++k) {
            const bool in = is_inl[(size_t)k] != 0;
            if (in == (invert != 0)) plane_pc.push_back(cloud[(size_t)k]); else leftover.push_back(cloud[(size_t)k]);
        }
        // pcl::compute3DCentroid: sequential float32 sums, then one division per component
        float cs[3] = {0.f, 0.f, 0.f};
        for (const P3& q3 : plane_pc) { cs[0] += q3.x; cs[1] += q3.y; cs[2] += q3.z; }
        const float cnt = (float)plane_pc.size();
        for (int a = 0; a < 3; ++a) mids[i][a] = cs[a] / cnt;
        mids[i][3] = 0.f;
        normals[i][0] = c->h_model[0].x; normals[i][1] = c->h_model[0].y; normals[i][2] = c->h_model[0].z; normals[i][3] = c->h_model[0].w;
        counts[i] = (int)plane_pc.size();
        cloud.swap(leftover);
    }
    // sne.cpp:199-212: order by size (the callback's own exchange loops), largest first
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j)
            if (counts[i] < counts[j]) {
                std::swap(counts[i], counts[j]);
                for (int a = 0; a < 4; ++a) { std::swap(normals[i][a], normals[j][a]); std::swap(mids[i][a], mids[j][a]); }
            }
    hm::surface_frame(normals, mids, out->Rt);
    for (int i = 0; i < 3; ++i) {
        out->n_points[i] = counts[i];
        for (int a = 0; a < 4; ++a) { out->coeff[i][a] = normals[i][a]; out->midpoint[i][a] = mids[i][a]; }
    }
    return CD_OK;
}

// cd_surface_frame over a batch: the records go up as they are, k_surface_load unpacks them on the device (no host loop over
// points) and stage_surface runs the three fits of every frame together
static int cd_surface_batch_impl(cd_context* c, const void* xyz, size_t stride, int P, const int32_t* n_points, int F,
                                 const float* table_normals, int invert, const cd_params* p, cd_surface_frame_result* out, int32_t* status) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!n_points || !table_normals || !out || !status || F <= 0 || P < 0 || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    int max_n = 0;
    for (int f = 0; f < F; ++f) {
        if (n_points[f] < 0 || n_points[f] > P) return fail(c, CD_ERR_INVALID_ARG, "n_points[f] outside [0, points_per_frame]");
        max_n = std::max(max_n, (int)n_points[f]);
    }
    if (max_n > 0 && !xyz) return fail(c, CD_ERR_INVALID_ARG, "xyz is NULL");
    if (F > c->F || max_n > c->N) return fail(c, CD_ERR_CAPACITY, "batch larger than the context capacity");
    const int pitch = std::max(max_n, 1);
    st = ensure_surface(c, (size_t)pitch);
    if (st) return st;
    std::vector<int> count(n_points, n_points + F);
    for (int f = 0; f < F; ++f) {
        std::memset(&c->h_sfs[f], 0, sizeof(FrameState));
        c->h_sfs[f].n_v = count[(size_t)f];
    }
    HIPCHK(c, xfer(c, c->d_sfs, c->h_sfs, sizeof(FrameState) * F, hipMemcpyHostToDevice));
    if (max_n > 0) {
        const size_t bytes = ((size_t)(F - 1) * P + (size_t)n_points[F - 1]) * stride;
        st = ensure_input(c, std::max<size_t>(bytes, 16));
        if (st) return st;
        if (bytes > 0) HIPCHK(c, hipMemcpyAsync(c->d_in, xyz, bytes, hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, launch_surface_load(c->stream, c->d_in, stride, stride * (size_t)P, (const int*)((char*)c->d_sfs.get() + offsetof(FrameState, n_v)),
                                      FS_PITCH, pitch, max_n, F, c->d_spts[0]));
    }
    const std::vector<char> run((size_t)F, 1);
    return stage_surface(c, F, pitch, count, table_normals, run, invert, p, out, status);
}

static int cd_bbox_filter_impl(cd_context* c, const void* xyz, size_t stride, int n, const double P[12], const int32_t rect[4],
                   int32_t* out_indices, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    if ((!xyz && n > 0) || !P || !rect || !out_indices || !out_n || n < 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (n == 0) return CD_OK;
    int st = load_as(c, xyz, stride, n, c->d_vox, &FrameState::n_v);
    if (st) return st;
    cd_params q;
    cd_default_params(&q);
    for (int i = 0; i < 12; ++i) q.bbox_P[i] = P[i];
    for (int i = 0; i < 4; ++i) q.bbox_rect[i] = rect[i];
    HIPCHK(c, hipMemsetAsync(c->d_have, 0, sizeof(int), c->stream));
    c->h_active[0] = 0;   // (no plane: with mirror reads the kernels look here; no kernel of this context is in flight)
    st = stage_extract(c, 1, &q, 2);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const int ni = c->h_fs[0].n_plane;
    if (ni > capacity) return fail(c, CD_ERR_CAPACITY, "index capacity too small");
    if (ni > 0) HIPCHK(c, copy_sync(c, out_indices, c->d_plane_idx, sizeof(int) * ni, hipMemcpyDeviceToHost));
    *out_n = ni;
    return CD_OK;
}

static int cd_extract_impl(cd_context* c, const void* points, size_t stride, int n, const int32_t* indices, int n_indices, int negative,
               void* out_points, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    if ((!points && n > 0) || (!indices && n_indices > 0) || !out_n || n < 0 || n_indices < 0 || capacity < 0 || stride < 4 || (stride & 3) ||
        (!out_points && capacity > 0))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (n > c->N || (!negative && n_indices > c->N)) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (n == 0) return CD_OK;
    const int words = (int)(stride / 4);
    // staging buffer: the input records, then room for the records that are kept
    const size_t in_bytes = ((size_t)n * stride + 255) & ~(size_t)255;
    int st = ensure_input(c, in_bytes + (size_t)(negative ? n : n_indices) * stride);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, (size_t)n * stride, hipMemcpyHostToDevice, c->stream));
    // index list -> d_label (upload), kept indices -> d_plane_idx
    const int mi = std::min(n_indices, c->N);
    if (mi > 0) HIPCHK(c, hipMemcpyAsync(c->d_label, indices, sizeof(int) * (size_t)mi, hipMemcpyHostToDevice, c->stream));
    int kept = 0;
    const int* d_keep = c->d_label;
    if (negative) {
        if (n_indices > c->N) return fail(c, CD_ERR_CAPACITY, "index list longer than the context capacity");
        std::memset(&c->h_fs[0], 0, sizeof(FrameState));
        HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemsetAsync(c->d_rank, 0, sizeof(int) * (size_t)n, c->stream));            // marks
        HIPCHK(c, hipMemsetAsync(c->d_tileA, 0, sizeof(int) * (size_t)c->T, c->stream));          // chained-scan state
        HIPCHK(c, hipMemsetAsync(c->d_ticket, 0, sizeof(int), c->stream));
        LAUNCH(c, launch_mark_indices(c->stream, c->d_label, mi, n, c->d_rank));
        LAUNCH(c, launch_select_unmarked(c->stream, c->d_rank, n, c->d_tileA, c->d_fs, c->d_plane_idx, c->d_ticket));
        st = sync_fs(c, 1);
        if (st) return st;
        kept = c->h_fs[0].n_plane;
        d_keep = c->d_plane_idx;
    } else {
        for (int i = 0; i < n_indices; ++i)
            if (indices[i] < 0 || indices[i] >= n) return fail(c, CD_ERR_INVALID_ARG, "index out of range");
        kept = n_indices;
    }
    if (kept > capacity) return fail(c, CD_ERR_CAPACITY, "output capacity too small");
    if (kept > 0) {
        char* d_out = (char*)c->d_in + in_bytes;
        LAUNCH(c, launch_gather_records(c->stream, c->d_in, words, d_keep, kept, d_out));
        HIPCHK(c, copy_sync(c, out_points, d_out, (size_t)kept * stride, hipMemcpyDeviceToHost));
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // the uploads read caller memory
    }
    *out_n = kept;
    return CD_OK;
}

static int cd_passthrough_impl(cd_context* c, const void* points, size_t stride, int n, int field, double lo, double hi, int negative,
                               void* out_points, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    if ((!points && n > 0) || !out_n || n < 0 || capacity < 0 || stride < 12 || (stride & 3) || (!out_points && capacity > 0) || field < -1 || field > 2)
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (n == 0) return CD_OK;
    const int words = (int)(stride / 4);
    const size_t in_bytes = ((size_t)n * stride + 255) & ~(size_t)255;   // staging: the input records, then the records that are kept
    int st = ensure_input(c, in_bytes + (size_t)n * stride);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, (size_t)n * stride, hipMemcpyHostToDevice, c->stream));
    std::memset(&c->h_fs[0], 0, sizeof(FrameState));
    HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_tileA, 0, sizeof(int) * (size_t)c->T, c->stream));          // chained-scan state
    HIPCHK(c, hipMemsetAsync(c->d_ticket, 0, sizeof(int), c->stream));
    LAUNCH(c, launch_passthrough_mark(c->stream, c->d_in, stride, n, field < 0 ? -1 : 4 * field, lo, hi, negative ? 1 : 0, c->d_rank));
    LAUNCH(c, launch_select_unmarked(c->stream, c->d_rank, n, c->d_tileA, c->d_fs, c->d_plane_idx, c->d_ticket));
    st = sync_fs(c, 1);
    if (st) return st;
    const int kept = c->h_fs[0].n_plane;
    if (kept > capacity) return fail(c, CD_ERR_CAPACITY, "output capacity too small");
    if (kept > 0) {
        char* d_out = (char*)c->d_in + in_bytes;
        LAUNCH(c, launch_gather_records(c->stream, c->d_in, words, c->d_plane_idx, kept, d_out));
        HIPCHK(c, copy_sync(c, out_points, d_out, (size_t)kept * stride, hipMemcpyDeviceToHost));
    }
    *out_n = kept;
    return CD_OK;
}

static int cd_cluster_impl(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, int32_t* labels,
               int32_t* sizes, int sizes_capacity, int* out_k) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!xyz || !labels || n < 0 || stride < 12 || (sizes_capacity > 0 && !sizes)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (out_k) *out_k = 0;
    if (n == 0) return CD_OK;
    st = load_as(c, xyz, stride, n, c->d_obj, &FrameState::n_o);
    if (st) return st;
    st = stage_cluster_sync(c, 1, p, n);
    if (st) return st;
    HIPCHK(c, copy_sync(c, labels, c->d_label, sizeof(int) * n, hipMemcpyDeviceToHost));
    const int K = c->h_fs[0].n_k;
    const int ks = std::min(K, sizes_capacity);
    if (ks > 0) HIPCHK(c, copy_sync(c, sizes, c->d_sizes, sizeof(int) * ks, hipMemcpyDeviceToHost));
    if (out_k) *out_k = K;
    return CD_OK;
}

static int cd_icp_impl(cd_context* c, int slot, const void* src_xyz, size_t stride, int n, const cd_params* p,
           cd_cluster_result* out, float* aligned) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!src_xyz || !out || n < 0 || stride < 12 || slot < 0 || slot >= CD_MAX_TEMPLATES) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (p->icp_use_guess == CD_GUESS_SURFACE) return fail(c, CD_ERR_INVALID_ARG, "icp_use_guess = CD_GUESS_SURFACE needs a frame to fit: fused calls only");
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (c->tpl_m[slot] <= 0) return fail(c, CD_ERR_NO_TEMPLATE, "template slot is empty");
    st = upload_points(c, src_xyz, stride, n, c->d_src0);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_src, c->d_src0, sizeof(float4) * (size_t)std::max(n, 1), hipMemcpyDeviceToDevice, c->stream));
    const int off0 = 0;
    set_icp_clusters(c, 0, 1, 0, &n, &off0, 0, slot);
    st = stage_icp(c, 1, p, nullptr);
    if (st) return st;
    fill_cluster_result(c, 0, p, out);
    out->template_slot = slot;
    if (aligned && n > 0) {
        std::vector<float4> tmp((size_t)n);
        HIPCHK(c, copy_sync(c, tmp.data(), c->d_src, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) { aligned[3 * i] = tmp[i].x; aligned[3 * i + 1] = tmp[i].y; aligned[3 * i + 2] = tmp[i].z; }
    }
    // rule C8: an ICP that stopped for fewer than three kept correspondences (only a bounded one can: every other ends converged)
    if (c->h_st[0].status == CD_OK && c->icp_bounded && !c->h_st[0].converged) return CD_ERR_FEW_CORRESPONDENCES;
    return c->h_st[0].status;
}

static int cd_process_batch_device_impl(cd_context* c, const void* d_frames, size_t stride, int points_per_frame, int n_frames,
                            const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    return process_batch_impl(c, d_frames, stride, points_per_frame, n_frames, p, results, plane_inliers, labels);
}

static int cd_process_batch_impl(cd_context* c, const void* frames, size_t stride, int points_per_frame, int n_frames,
                     const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!frames || points_per_frame <= 0 || n_frames <= 0) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    const size_t bytes = (size_t)points_per_frame * n_frames * stride;
    int st = check_bbox_source(c, p, n_frames, false);   // (before the upload)
    if (st) return st;
    st = ensure_input(c, bytes);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, frames, bytes, hipMemcpyHostToDevice, c->stream));
    return process_batch_impl(c, c->d_in, stride, points_per_frame, n_frames, p, results, plane_inliers, labels);
}

int cd_process_frame(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, cd_frame_result* result,
                     int32_t* plane_inliers, int32_t* labels) {
    return cd_process_batch(c, points, stride, n, 1, p, result, plane_inliers, labels);
}

int cd_get_cluster_results(const cd_context* c, int frame, int first, int capacity, cd_cluster_result* out, int* out_total) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (out_total) *out_total = 0;
    if (frame < 0 || first < 0 || capacity < 0 || (capacity > 0 && !out)) return CD_ERR_INVALID_ARG;
    if ((size_t)frame + 1 >= c->last_first.size()) return CD_ERR_INVALID_ARG;   // not a frame of the last batch
    const int lo = c->last_first[(size_t)frame], hi = c->last_first[(size_t)frame + 1];
    if (lo < 0 || hi < lo || (size_t)hi > c->last_clusters.size()) return CD_ERR_INVALID_ARG;
    if (out_total) *out_total = hi - lo;
    int n = 0;
    for (int k = lo + first; k < hi && n < capacity; ++k) out[n++] = c->last_clusters[(size_t)k];
    return n;
}

// float4 points on the device -> `m` records of `stride` bytes in caller memory (k_pack_records, then ONE download).
// The staging area is the context's input buffer (its contents - the frames of a host-pointer call - are dead by now).
static int download_records(cd_context* c, const float4* d_pts, int m, size_t stride, int rgb_offset, uint32_t pad3, void* out,
                            size_t staging_skip = 0) {
    if (m <= 0) return CD_OK;
    const size_t skip = (staging_skip + 255) & ~(size_t)255;
    int st = CD_OK;
    if (skip + (size_t)m * stride > c->d_in.capacity()) {
        if (skip) return fail(c, CD_ERR_CAPACITY, "record staging area too small");   // (callers that keep the input size the buffer beforehand)
        st = ensure_input(c, (size_t)m * stride);
        if (st) return st;
    }
    char* d_out = c->d_in + skip;
    LAUNCH(c, launch_pack_records(c->stream, d_pts, m, (int)(stride / 4), rgb_offset >= 0 ? rgb_offset / 4 : -1, pad3, d_out));
    HIPCHK(c, copy_sync(c, out, d_out, (size_t)m * stride, hipMemcpyDeviceToHost));
    return CD_OK;
}

// ---- depth-image input (k_depth.hip) ---------------------------------------------------------------------------------------
// every check of the header's list, before anything is copied or launched
static int check_depth(cd_context* c, const cd_depth_camera* cam, const void* depth, const void* color, int n_frames) {
    if (!cam) return fail(c, CD_ERR_INVALID_ARG, "depth camera is NULL");
    if (!depth) return fail(c, CD_ERR_INVALID_ARG, "depth image is NULL");
    if (cam->width <= 0 || cam->height <= 0 || (long long)cam->width * cam->height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    if (cam->color != CD_COLOR_NONE && cam->color != CD_COLOR_RGB8) return fail(c, CD_ERR_INVALID_ARG, "unknown colour mode");
    if (cam->color == CD_COLOR_RGB8 && !color) return fail(c, CD_ERR_INVALID_ARG, "colour requested with a NULL colour image");
    for (float v : {cam->fx, cam->fy, cam->depth_scale})
        if (!(std::isfinite(v) && v > 0.f)) return fail(c, CD_ERR_INVALID_ARG, "fx, fy and depth_scale must be finite and > 0");
    return CD_OK;
}

static_assert(sizeof(cd_color_camera) == 80 && offsetof(cd_color_camera, no_texture) == 72, "cd_color_camera has no padding holes");
// what a mapped call (rule C12) needs besides check_depth: nullptr = fine, else what is wrong (shared with the host-only
// cd_texture_project)
static const char* color_camera_error(const cd_color_camera* cc) {
    if (!cc) return "colour camera is NULL";
    if (cc->width <= 0 || cc->height <= 0) return "the colour image's width * height must be in 1 .. the context's max_points";
    for (float v : {cc->fx, cc->fy})
        if (!(std::isfinite(v) && v > 0.f)) return "the colour camera's fx and fy must be finite and > 0";
    for (float v : {cc->cx, cc->cy})
        if (!std::isfinite(v)) return "the colour camera's cx or cy is not finite";
    for (float v : cc->R) if (!std::isfinite(v)) return "R holds a non-finite value";
    for (float v : cc->t) if (!std::isfinite(v)) return "t holds a non-finite value";
    if (cc->no_texture != CD_NOTEX_DROP && cc->no_texture != CD_NOTEX_KEEP) return "unknown no_texture mode";
    return nullptr;
}

// every check of the header's list for a mapped call, before anything is copied or launched
static int check_mapped(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* cc, const void* depth, const void* color, int n_frames) {
    int st = check_depth(c, cam, depth, color, n_frames);
    if (st) return st;
    if (cam->color != CD_COLOR_RGB8) return fail(c, CD_ERR_INVALID_ARG, "a mapped call needs CD_COLOR_RGB8");
    if (const char* msg = color_camera_error(cc)) return fail(c, CD_ERR_INVALID_ARG, msg);
    if ((long long)cc->width * cc->height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "the colour image's width * height must be in 1 .. the context's max_points");
    return CD_OK;
}

// host images -> the context's depth / colour buffers (one copy each, on the context's stream); ccam: the colour images have
// their own size
static int upload_depth(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, int n_frames, DepthJob* dj,
                        const cd_color_camera* ccam = nullptr) {
    const size_t px = (size_t)cam->width * cam->height * n_frames;
    const size_t cpx = ccam ? (size_t)ccam->width * ccam->height * n_frames : px;
    GROW(c, d_depth, (size_t)c->N * c->F);
    HIPCHK(c, hipMemcpyAsync(c->d_depth, depth, px * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    dj->cam = cam;
    dj->depth = c->d_depth;
    dj->color = nullptr;
    if (cam->color == CD_COLOR_RGB8) {
        GROW(c, d_color, (size_t)c->N * c->F * 3);
        HIPCHK(c, hipMemcpyAsync(c->d_color, color, cpx * 3, hipMemcpyHostToDevice, c->stream));
        dj->color = c->d_color;
    }
    dj->ccam = ccam;
    return CD_OK;
}

// ccam != nullptr: the mapped call (rule C12)
static int cd_process_depth_batch_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, int n_frames,
                                       const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels, bool on_device,
                                       const cd_color_camera* ccam = nullptr, bool mapped = false) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    int st = check_params(c, p);
    if (st) return st;
    if (!results) return fail(c, CD_ERR_INVALID_ARG, "results is NULL");
    st = mapped ? check_mapped(c, cam, ccam, depth, color, n_frames) : check_depth(c, cam, depth, color, n_frames);
    if (st) return st;
    st = check_bbox_source(c, p, n_frames, cam->color == CD_COLOR_RGB8);   // (before the uploads)
    if (st) return st;
    cd_params q = *p;
    q.rgb_offset = cam->color == CD_COLOR_RGB8 ? 12 : -1;   // the canonical records: x y z rgb, 16 bytes
    const int P = cam->width * cam->height;
    st = ensure_input(c, (size_t)P * n_frames * sizeof(float4));
    if (st) return st;
    DepthJob dj{cam, depth, cam->color == CD_COLOR_RGB8 ? color : nullptr, ccam};
    if (!on_device) {
        st = upload_depth(c, cam, depth, color, n_frames, &dj, ccam);
        if (st) return st;
    }
    return process_batch_impl(c, c->d_in, sizeof(float4), P, n_frames, &q, results, plane_inliers, labels, &dj);
}

static int cd_depth_to_cloud_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, void* out_records,
                                  size_t stride, int rgb_offset, int capacity, int* out_n, const cd_color_camera* ccam = nullptr,
                                  bool mapped = false) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!out_n || capacity < 0 || (capacity > 0 && !out_records) || stride < 12 || (stride & 3) ||
        (rgb_offset >= 0 && (rgb_offset < 12 || (rgb_offset & 3) || (size_t)rgb_offset + 4 > stride)))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    int st = mapped ? check_mapped(c, cam, ccam, depth, color, 1) : check_depth(c, cam, depth, color, 1);
    if (st) return st;
    *out_n = 0;
    invalidate_last(c);
    const int P = cam->width * cam->height;
    if (P > capacity) { *out_n = P; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    // one buffer: the canonical records, then (256-byte aligned) the caller's layout that goes back
    const size_t rec_bytes = (size_t)P * sizeof(float4);
    st = ensure_input(c, ((rec_bytes + 255) & ~(size_t)255) + (size_t)P * stride);
    if (st) return st;
    DepthJob dj;
    st = upload_depth(c, cam, depth, color, 1, &dj, ccam);
    if (st) return st;
    LAUNCH(c, launch_depth_job(c->stream, &dj, 1, reinterpret_cast<float4*>(c->d_in.get())));
    st = download_records(c, reinterpret_cast<const float4*>(c->d_in.get()), P, stride, rgb_offset, 0u, out_records, rec_bytes);
    if (st) return st;
    *out_n = P;
    return CD_OK;
}

// ---- colour gate as a call of its own (rule C10) ------------------------------------------------------------------------------
static int cd_color_bbox_batch_impl(cd_context* c, const uint8_t* rgb8, int width, int height, int n_frames, const cd_color_gate_params* g,
                                    cd_color_bbox* out, bool on_device) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!rgb8 || !out) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (width <= 0 || height <= 0 || (long long)width * height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    cd_color_gate_params def;
    cd_default_color_gate_params(&def);
    if (!g) g = &def;
    int st = check_color_params(c, g);
    if (st) return st;
    invalidate_last(c);
    const uint8_t* d_rgb = rgb8;
    if (!on_device) {
        GROW(c, d_color, (size_t)c->N * c->F * 3);
        HIPCHK(c, hipMemcpyAsync(c->d_color, rgb8, (size_t)width * height * n_frames * 3, hipMemcpyHostToDevice, c->stream));
        d_rgb = c->d_color;
    }
    st = stage_color(c, d_rgb, width, height, n_frames, g);
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_crec, sizeof(cd_color_bbox) * (size_t)n_frames);
    return color_status(c, n_frames);
}

// ---- overlay (rule C11, k_overlay.hip) -----------------------------------------------------------------------------------------
static_assert(sizeof(OverlayBox) == sizeof(cd_overlay_box) && offsetof(cd_overlay_box, drawn) == offsetof(OverlayBox, drawn), "the kernel's record is cd_overlay_box");
static_assert(sizeof(cd_overlay_params) == 12 * 8 + 16 * 8 + 3 * 8 + 4 + 4 + 6 * 4 && offsetof(cd_overlay_params, reserved) == 256, "cd_overlay_params has no padding holes");
constexpr int OVERLAY_MAX_BOXES = 1024;   // boxes_per_frame of a draw call

// the checks on the parameters alone (shared with the host-only cd_overlay_project): nullptr = fine, else what is wrong
static const char* overlay_params_error(const cd_overlay_params* op) {
    for (double v : op->P) if (!std::isfinite(v)) return "P holds a non-finite value";
    for (double v : op->E) if (!std::isfinite(v)) return "E holds a non-finite value";
    for (double v : op->dims) if (!std::isfinite(v)) return "dims holds a non-finite value";
    if (op->thickness < 1 || op->thickness > OVERLAY_MAX_THICKNESS) return "thickness must be in 1 .. 64";
    return nullptr;
}

// rule C11 step 2: M = P E, every entry ((p0 e0 + p1 e1) + p2 e2) + p3 e3
static OverlayParams overlay_kernel_params(const cd_overlay_params* op) {
    OverlayParams k;
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col)
            k.M[4 * r + col] = ((op->P[4 * r] * op->E[col] + op->P[4 * r + 1] * op->E[4 + col]) + op->P[4 * r + 2] * op->E[8 + col]) + op->P[4 * r + 3] * op->E[12 + col];
    for (int i = 0; i < 3; ++i) k.dims[i] = op->dims[i];
    return k;
}

// every check of the header's list but those on n_boxes, before anything is copied or launched
static int check_overlay(cd_context* c, const void* rgb8, int width, int height, int n_frames, const cd_overlay_params* op, const void* out) {
    if (!rgb8 || !out) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (width <= 0 || height <= 0 || (long long)width * height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (width > OVERLAY_COORD_MAX || height > OVERLAY_COORD_MAX) return fail(c, CD_ERR_INVALID_ARG, "width and height must not exceed 8192");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    if (const char* msg = overlay_params_error(op)) return fail(c, CD_ERR_INVALID_ARG, msg);
    return CD_OK;
}

// poses (F * B * 16 doubles) and n_boxes (F) are HOST memory; img is device memory (on_device) or host memory that is
// uploaded, drawn on and downloaded again.  Leaves the read-back state of the last fused call alone.
static int stage_overlay(cd_context* c, uint8_t* img, int W, int H, int F, const double* poses, const int32_t* n_boxes, int B,
                         const cd_overlay_params* op, cd_overlay_box* out, bool on_device) {
    const size_t nb = (size_t)F * (size_t)B;
    GROW(c, d_oposes, nb * 16); GROW(c, d_obox, nb); GROW(c, h_obox, nb);
    GROW(c, d_onbox, (size_t)c->F);
    const size_t img_bytes = (size_t)W * H * F * 3;
    uint8_t* d_img = img;
    if (!on_device) {
        GROW(c, d_color, (size_t)c->N * c->F * 3);
        HIPCHK(c, hipMemcpyAsync(c->d_color, img, img_bytes, hipMemcpyHostToDevice, c->stream));
        d_img = c->d_color;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_oposes, poses, sizeof(double) * 16 * nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_onbox, n_boxes, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, c->stream));
    const OverlayParams kp = overlay_kernel_params(op);
    LAUNCH(c, launch_overlay_project(c->stream, c->d_oposes, c->d_onbox, B, F, kp, c->d_obox));
    LAUNCH(c, launch_overlay_raster(c->stream, d_img, W, H, B, F, op->thickness, op->rgb, c->d_obox));
    HIPCHK(c, hipMemcpyAsync(c->h_obox, c->d_obox, sizeof(OverlayBox) * nb, hipMemcpyDeviceToHost, c->stream));
    if (!on_device) HIPCHK(c, hipMemcpyAsync(img, d_img, img_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_obox, sizeof(cd_overlay_box) * nb);
    return CD_OK;
}

static int cd_draw_boxes_batch_impl(cd_context* c, uint8_t* rgb8, int width, int height, int n_frames, const double* poses,
                                    const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* op, cd_overlay_box* out, bool on_device) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    cd_overlay_params def;
    cd_default_overlay_params(&def);
    if (!op) op = &def;
    int st = check_overlay(c, rgb8, width, height, n_frames, op, out);
    if (st) return st;
    if (!poses || !n_boxes) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (boxes_per_frame < 1 || boxes_per_frame > OVERLAY_MAX_BOXES) return fail(c, CD_ERR_INVALID_ARG, "boxes_per_frame must be in 1 .. 1024");
    for (int f = 0; f < n_frames; ++f)
        if (n_boxes[f] < 0 || n_boxes[f] > boxes_per_frame) return fail(c, CD_ERR_INVALID_ARG, "n_boxes[f] must be in 0 .. boxes_per_frame");
    invalidate_last(c);
    return stage_overlay(c, rgb8, width, height, n_frames, poses, n_boxes, boxes_per_frame, op, out, on_device);
}

static int cd_draw_last_results_impl(cd_context* c, uint8_t* rgb8, int width, int height, int which, const cd_overlay_params* op,
                                     cd_overlay_box* out, bool on_device) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    cd_overlay_params def;
    cd_default_overlay_params(&def);
    if (!op) op = &def;
    if (c->last_first.size() < 2) return fail(c, CD_ERR_INVALID_ARG, "no fused call to draw: none has run, or another compute call has run since");
    const int F = (int)c->last_first.size() - 1;
    int st = check_overlay(c, rgb8, width, height, F, op, out);
    if (st) return st;
    if (which != CD_DRAW_ACCEPTED && which != CD_DRAW_ALL) return fail(c, CD_ERR_INVALID_ARG, "unknown selection of boxes");
    // slot k of frame f = cluster k of its record; a slot that is not drawn carries a NaN pose, which rule C11 skips
    constexpr int B = CD_MAX_CLUSTERS_PER_FRAME;
    std::vector<double> poses((size_t)F * B * 16, std::numeric_limits<double>::quiet_NaN());
    std::vector<int32_t> n_boxes((size_t)F, 0);
    for (int f = 0; f < F; ++f) {
        const int lo = c->last_first[(size_t)f], hi = c->last_first[(size_t)f + 1];
        if (lo < 0 || hi < lo || (size_t)hi > c->last_clusters.size()) return fail(c, CD_ERR_INVALID_ARG, "no fused call to draw");
        const int n = std::min(hi - lo, B);
        n_boxes[(size_t)f] = n;
        for (int k = 0; k < n; ++k) {
            const cd_cluster_result& cr = c->last_clusters[(size_t)(lo + k)];
            if (which == CD_DRAW_ALL || cr.accepted) std::memcpy(&poses[((size_t)f * B + k) * 16], cr.pose, sizeof(cr.pose));
        }
    }
    return stage_overlay(c, rgb8, width, height, F, poses.data(), n_boxes.data(), B, op, out, on_device);
}

// ---- pose verification (rule C14, k_verify.hip) -----------------------------------------------------------------------------------
static_assert(sizeof(VerifyRecord) == sizeof(cd_verify_box) && sizeof(cd_verify_box) == 48 && offsetof(cd_verify_box, agree_abs_um) == offsetof(VerifyRecord, agree_abs_um) &&
              offsetof(cd_verify_box, score) == 40, "the kernel's record is cd_verify_box");
static_assert(sizeof(cd_verify_params) == (3 + 3 * CD_MAX_TEMPLATES + 2) * 8 + 8 * 4 && offsetof(cd_verify_params, reserved) == sizeof(cd_verify_params) - 24, "cd_verify_params has no padding holes");
static_assert(sizeof(VerifyJob) == 152, "152 bytes per box cross the bus");

static bool verify_dim_ok(double v) { return std::isfinite(v) && v >= 0.0; }
// the checks on the camera and the parameters alone (shared with the host-only entries): nullptr = fine, else what is wrong
static const char* verify_camera_error(const cd_depth_camera* cam) {
    if (!cam) return "depth camera is NULL";
    if (cam->color != CD_COLOR_NONE && cam->color != CD_COLOR_RGB8) return "unknown colour mode";
    for (float v : {cam->fx, cam->fy, cam->depth_scale})
        if (!(std::isfinite(v) && v > 0.f)) return "fx, fy and depth_scale must be finite and > 0";
    return nullptr;
}
static const char* verify_params_error(const cd_verify_params* vp) {
    for (double v : vp->dims) if (!verify_dim_ok(v)) return "dims must be finite and >= 0";
    if (vp->use_slot_dims)
        for (int s = 0; s < CD_MAX_TEMPLATES; ++s)
            for (double v : vp->slot_dims[s]) if (!verify_dim_ok(v)) return "slot_dims must be finite and >= 0";
    if (!verify_dim_ok(vp->tolerance)) return "tolerance must be finite and >= 0";
    if (!std::isfinite(vp->min_score)) return "min_score must be finite";
    if (vp->min_agree < 0) return "min_agree must be >= 0";
    return nullptr;
}
static VerifyCam verify_kernel_camera(const cd_depth_camera* cam) {
    VerifyCam k;
    k.fx = (double)cam->fx; k.fy = (double)cam->fy; k.cx = (double)cam->cx; k.cy = (double)cam->cy; k.depth_scale = (double)cam->depth_scale;
    k.width = cam->width; k.height = cam->height;
    return k;
}
// rule C14 step 5: what the host adds to the counts
static void verify_finish(const cd_verify_params* vp, cd_verify_box* r) {
    const long long den = (long long)r->n_agree + (long long)r->n_through;
    r->score = den != 0 ? (double)r->n_agree / (double)den : 0.0;
    r->passed = (r->verified && r->n_agree >= vp->min_agree && r->score >= vp->min_score) ? 1 : 0;
    r->reserved = 0;
}

// every check of the header's list but those on the boxes, before anything is copied or launched
static int check_verify(cd_context* c, const cd_depth_camera* cam, const void* depth, int n_frames, const cd_verify_params* vp, const void* out) {
    if (!depth || !out) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (const char* msg = verify_camera_error(cam)) return fail(c, CD_ERR_INVALID_ARG, msg);
    if (cam->width <= 0 || cam->height <= 0 || (long long)cam->width * cam->height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    if (const char* msg = verify_params_error(vp)) return fail(c, CD_ERR_INVALID_ARG, msg);
    return CD_OK;
}

// poses (F * B * 16 doubles), n_boxes (F) and dims (F * B * 3 doubles) are HOST memory; depth is device memory (on_device) or host
// memory that is uploaded into d_vdepth.  Reads the images only, and leaves the read-back state of the last fused call alone.
static int stage_verify(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int F, const double* poses, const int32_t* n_boxes,
                        int B, const double* dims, const cd_verify_params* vp, cd_verify_box* out, bool on_device) {
    const size_t nb = (size_t)F * (size_t)B;
    GROW(c, d_vjob, nb); GROW(c, h_vjob, nb); GROW(c, d_vrec, nb); GROW(c, h_vrec, nb);
    GROW(c, d_vnbox, (size_t)c->F); GROW(c, h_vnbox, (size_t)c->F);
    const uint16_t* d_img = depth;
    if (!on_device) {
        const size_t px = (size_t)cam->width * cam->height * F;
        GROW(c, d_vdepth, px);
        HIPCHK(c, hipMemcpyAsync(c->d_vdepth, depth, px * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        d_img = c->d_vdepth;
    }
    for (int f = 0; f < F; ++f) {
        c->h_vnbox[f] = n_boxes[f];
        for (int b = 0; b < B; ++b) {
            const size_t i = (size_t)f * B + b;
            VerifyJob& j = c->h_vjob[i];
            std::memcpy(j.pose, poses + i * 16, sizeof(j.pose));
            std::memcpy(j.dims, dims + i * 3, sizeof(j.dims));
        }
    }
    HIPCHK(c, hipMemcpyAsync(c->d_vjob, c->h_vjob, sizeof(VerifyJob) * nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_vnbox, c->h_vnbox, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, launch_verify_boxes(c->stream, d_img, verify_kernel_camera(cam), vp->tolerance, c->d_vjob, c->d_vnbox, B, F, c->d_vrec));
    HIPCHK(c, hipMemcpyAsync(c->h_vrec, c->d_vrec, sizeof(VerifyRecord) * nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_vrec, sizeof(cd_verify_box) * nb);
    for (int f = 0; f < F; ++f)
        for (int b = 0; b < n_boxes[f]; ++b) verify_finish(vp, out + (size_t)f * B + b);
    return CD_OK;
}

static int cd_verify_boxes_batch_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, const double* poses,
                                      const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* vp,
                                      cd_verify_box* out, bool on_device) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    int st = check_verify(c, cam, depth, n_frames, vp, out);
    if (st) return st;
    if (!poses || !n_boxes) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (boxes_per_frame < 1 || boxes_per_frame > OVERLAY_MAX_BOXES) return fail(c, CD_ERR_INVALID_ARG, "boxes_per_frame must be in 1 .. 1024");
    const int B = boxes_per_frame;
    for (int f = 0; f < n_frames; ++f)
        if (n_boxes[f] < 0 || n_boxes[f] > B) return fail(c, CD_ERR_INVALID_ARG, "n_boxes[f] must be in 0 .. boxes_per_frame");
    std::vector<double> dims((size_t)n_frames * B * 3);
    for (size_t i = 0; i < (size_t)n_frames * B; ++i)
        for (int k = 0; k < 3; ++k) dims[i * 3 + k] = vp->dims[k];
    if (box_dims)
        for (int f = 0; f < n_frames; ++f)
            for (int b = 0; b < n_boxes[f]; ++b)
                for (int k = 0; k < 3; ++k) {
                    const size_t i = ((size_t)f * B + b) * 3 + k;
                    if (!verify_dim_ok(box_dims[i])) return fail(c, CD_ERR_INVALID_ARG, "box_dims must be finite and >= 0");
                    dims[i] = box_dims[i];
                }
    invalidate_last(c);
    return stage_verify(c, cam, depth, n_frames, poses, n_boxes, B, dims.data(), vp, out, on_device);
}

static int cd_verify_last_results_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int which, const cd_verify_params* vp,
                                       cd_verify_box* out, bool on_device) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    if (c->last_first.size() < 2) return fail(c, CD_ERR_INVALID_ARG, "no fused call to verify: none has run, or another compute call has run since");
    const int F = (int)c->last_first.size() - 1;
    int st = check_verify(c, cam, depth, F, vp, out);
    if (st) return st;
    if (which != CD_VERIFY_ACCEPTED && which != CD_VERIFY_ALL) return fail(c, CD_ERR_INVALID_ARG, "unknown selection of boxes");
    // slot k of frame f = cluster k of its record; a slot that is not selected carries a NaN pose (verified = 0, every count 0:
    // the zero record)
    constexpr int B = CD_MAX_CLUSTERS_PER_FRAME;
    std::vector<double> poses((size_t)F * B * 16, std::numeric_limits<double>::quiet_NaN());
    std::vector<double> dims((size_t)F * B * 3);
    std::vector<int32_t> n_boxes((size_t)F, 0);
    for (size_t i = 0; i < (size_t)F * B; ++i)
        for (int k = 0; k < 3; ++k) dims[i * 3 + k] = vp->dims[k];
    for (int f = 0; f < F; ++f) {
        const int lo = c->last_first[(size_t)f], hi = c->last_first[(size_t)f + 1];
        if (lo < 0 || hi < lo || (size_t)hi > c->last_clusters.size()) return fail(c, CD_ERR_INVALID_ARG, "no fused call to verify");
        const int n = std::min(hi - lo, B);
        n_boxes[(size_t)f] = n;
        for (int k = 0; k < n; ++k) {
            const cd_cluster_result& cr = c->last_clusters[(size_t)(lo + k)];
            if (which != CD_VERIFY_ALL && !cr.accepted) continue;
            const size_t i = (size_t)f * B + k;
            std::memcpy(&poses[i * 16], cr.pose, sizeof(cr.pose));
            if (vp->use_slot_dims && cr.template_slot >= 0 && cr.template_slot < CD_MAX_TEMPLATES)
                std::memcpy(&dims[i * 3], vp->slot_dims[cr.template_slot], 3 * sizeof(double));
        }
    }
    return stage_verify(c, cam, depth, F, poses.data(), n_boxes.data(), B, dims.data(), vp, out, on_device);
}

void cd_default_depth_camera(cd_depth_camera* cam) {
    if (!cam) return;
    std::memset(cam, 0, sizeof(*cam));
    cam->width = 640; cam->height = 480;                                  // README.md:74-75 of the reference
    cam->fx = cam->fy = 384.0898742675781f;                              // K[0], K[4] (README.md:78)
    cam->cx = 322.4656677246094f; cam->cy = 240.64073181152344f;        // K[2], K[5]
    cam->depth_scale = 0.001f;                                           // 16UC1 in millimetres (the RealSense driver's unit)
    cam->color = CD_COLOR_NONE;
}

void cd_default_color_camera(cd_color_camera* cc) {
    if (!cc) return;
    std::memset(cc, 0, sizeof(*cc));
    cc->width = 640; cc->height = 480;                                   // README.md:48-49 of the reference
    cc->fx = 616.8246459960938f; cc->fy = 616.609375f;                  // K[0], K[4] (README.md:52)
    cc->cx = 321.81976318359375f; cc->cy = 239.91116333007812f;         // K[2], K[5]
    cc->R[0] = cc->R[4] = cc->R[8] = 1.f;                                // the reference records no extrinsic values
    cc->no_texture = CD_NOTEX_DROP;
}

int cd_color_camera_struct_size(void) { return (int)sizeof(cd_color_camera); }

int cd_texture_project(const cd_depth_camera* cam, const cd_color_camera* cc, int u, int v, uint16_t d, float xyz[3], int32_t pix[2],
                       int32_t* textured) {
    if (!cam || color_camera_error(cc) || u < 0 || v < 0) return CD_ERR_INVALID_ARG;
    for (float f : {cam->fx, cam->fy, cam->depth_scale})
        if (!(std::isfinite(f) && f > 0.f)) return CD_ERR_INVALID_ARG;
    float q[3];
    int32_t px[2];
    const bool tex = texture_point(texture_params(cam, cc), (uint32_t)u, (uint32_t)v, d, q, px);
    if (xyz) std::memcpy(xyz, q, sizeof(q));
    if (pix) std::memcpy(pix, px, sizeof(px));
    if (textured) *textured = tex ? 1 : 0;
    return CD_OK;
}

int cd_get_frame_cloud(cd_context* c, int frame, int which, void* out_records, size_t stride, int rgb_offset, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!out_n || capacity < 0 || (capacity > 0 && !out_records) || stride < 12 || (stride & 3) || (which != CD_CLOUD_VOXELS && which != CD_CLOUD_OBJECTS) ||
        (rgb_offset >= 0 && (rgb_offset < 12 || (rgb_offset & 3) || (size_t)rgb_offset + 4 > stride)))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (!c->last_clouds || frame < 0 || (size_t)frame >= c->last_nv.size()) return fail(c, CD_ERR_INVALID_ARG, "not a frame of the last fused call of this context");
    const int m = which == CD_CLOUD_VOXELS ? c->last_nv[(size_t)frame] : c->last_no[(size_t)frame];
    if (m > capacity) { *out_n = m; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    const float4* src = (which == CD_CLOUD_VOXELS ? c->d_vox : c->d_obj) + (size_t)frame * c->N;
    const int st = download_records(c, src, m, stride, rgb_offset, 0u, out_records);
    if (st) return st;
    *out_n = m;
    return CD_OK;
}

int cd_get_cluster_points(cd_context* c, int frame, int k, int aligned, void* out_points, size_t stride, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!out_n || capacity < 0 || (capacity > 0 && !out_points) || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (!c->last_clouds || frame < 0 || (size_t)frame + 1 >= c->last_first.size()) return fail(c, CD_ERR_INVALID_ARG, "not a frame of the last fused call of this context");
    const int lo = c->last_first[(size_t)frame], hi = c->last_first[(size_t)frame + 1];
    if (k < 0 || lo + k >= hi || (size_t)(lo + k) >= c->last_clusters.size()) return fail(c, CD_ERR_INVALID_ARG, "no such cluster");
    const cd_cluster_result& r = c->last_clusters[(size_t)(lo + k)];
    const int m = r.size;
    if (m > capacity) { *out_n = m; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    const long long o0 = c->last_orig_off[(size_t)(lo + k)], o1 = c->last_al_off[(size_t)(lo + k)];
    const uint32_t one = 0x3f800000u;   // pcl::PointXYZ::data[3]
    int st;
    if (!aligned || o1 >= 0) {
        st = download_records(c, (aligned ? c->d_src : c->d_src0) + (aligned ? o1 : o0), m, stride, -1, one, out_points);
        if (st) return st;
    } else {
        // the pass that produced the best result has been overwritten by a later template pass: final_transformation * cluster
        st = download_records(c, c->d_src0 + o0, m, stride, -1, one, out_points);
        if (st) return st;
        for (int i = 0; i < m; ++i) {
            float v[3];
            char* rec = (char*)out_points + (size_t)i * stride;
            std::memcpy(v, rec, 12);
            const float* T = r.T;
            const float o[3] = {((T[0] * v[0] + T[1] * v[1]) + T[2] * v[2]) + T[3], ((T[4] * v[0] + T[5] * v[1]) + T[6] * v[2]) + T[7],
                                ((T[8] * v[0] + T[9] * v[1]) + T[10] * v[2]) + T[11]};
            std::memcpy(rec, o, 12);
        }
    }
    *out_n = m;
    return CD_OK;
}

static int cd_ground_plane_impl(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float coeff[4], void* out_records,
                    int capacity, int* out_n, int* out_n_inliers) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if ((!points && n > 0) || !coeff || !out_n || n < 0 || capacity < 0 || (capacity > 0 && !out_records) || stride < 12 || (stride & 3))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (out_n_inliers) *out_n_inliers = 0;
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (n == 0) return CD_ERR_NO_MODEL;
    // one buffer: the input blob, then (256-byte aligned) room for the records that go back
    const size_t in_bytes = (size_t)n * stride;
    st = ensure_input(c, ((in_bytes + 255) & ~(size_t)255) + in_bytes);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, in_bytes, hipMemcpyHostToDevice, c->stream));   // the ONE upload
    st = stage_crop_voxel(c, c->d_in, stride, n, 1, p, nullptr);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    if (c->h_fs[0].status != CD_OK) return fail(c, c->h_fs[0].status, "voxel grid: leaf size too small for the input extent");
    std::vector<int> iters;
    st = stage_plane(c, 1, p, iters, nullptr);
    if (st) return st;
    st = stage_extract(c, 1, p);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const int no = c->h_fs[0].n_o;
    if (out_n_inliers) *out_n_inliers = c->h_fs[0].n_plane;
    if (no > capacity) { *out_n = no; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    const int rgb_off = (p->rgb_offset >= 12 && !(p->rgb_offset & 3) && (size_t)p->rgb_offset + 4 <= stride) ? p->rgb_offset : -1;
    st = download_records(c, c->d_obj, no, stride, rgb_off, 0u, out_records, in_bytes);               // the ONE download
    if (st) return st;
    *out_n = no;
    if (!c->h_have[0]) return CD_ERR_NO_MODEL;
    coeff[0] = c->h_model[0].x; coeff[1] = c->h_model[0].y; coeff[2] = c->h_model[0].z; coeff[3] = c->h_model[0].w;
    return CD_OK;
}

// rule C8: the largest float32 f with (double)f <= d * d (one IEEE double multiply), and whether it bounds anything - it does
// not when d * d >= FLT_MAX, which no finite float d2 exceeds
int cd_icp_correspondence_threshold(double d, float* out_d2_max, int* out_bounded) {
    if (!(d >= 0.0)) return CD_ERR_INVALID_ARG;   // negative or NaN
    const double dd = d * d;
    float f = (float)dd;
    if ((double)f > dd) f = std::nextafter(f, 0.f);   // (rounded up: one float down; +inf above FLT_MAX comes down to FLT_MAX)
    if (out_d2_max) *out_d2_max = f;
    if (out_bounded) *out_bounded = dd >= (double)std::numeric_limits<float>::max() ? 0 : 1;
    return CD_OK;
}

int cd_set_icp_max_correspondence_distance(cd_context* c, double max_distance) {
    if (!c) return CD_ERR_INVALID_ARG;
    float d2 = 0.f;
    int bounded = 0;
    if (cd_icp_correspondence_threshold(max_distance, &d2, &bounded) != CD_OK)
        return fail(c, CD_ERR_INVALID_ARG, "the maximum correspondence distance is negative or NaN");
    c->icp_max_dist = max_distance;
    c->icp_d2_max = d2;
    c->icp_bounded = bounded;
    return CD_OK;
}

int cd_get_icp_max_correspondence_distance(const cd_context* c, double* out) {
    if (!c || !out) return CD_ERR_INVALID_ARG;
    *out = c->icp_max_dist;
    return CD_OK;
}

int cd_set_surface_distance_threshold(cd_context* c, double d) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (!std::isfinite(d) || !(d > 0.0)) return fail(c, CD_ERR_INVALID_ARG, "the surface distance threshold must be finite and > 0");
    c->surface_thr = d;
    return CD_OK;
}

int cd_get_surface_distance_threshold(const cd_context* c, double* out) {
    if (!c || !out) return CD_ERR_INVALID_ARG;
    *out = c->surface_thr;
    return CD_OK;
}

int cd_get_surface_results(const cd_context* c, int first, int capacity, cd_surface_frame_result* out, int32_t* frame_status) {
    if (!c || first < 0 || capacity < 0) return CD_ERR_INVALID_ARG;
    if (!c->last_surface_ok) return CD_ERR_INVALID_ARG;   // (no fused call in CD_GUESS_SURFACE mode since the last compute call)
    int n = 0;
    for (size_t f = (size_t)first; f < c->last_surface.size() && n < capacity; ++f, ++n) {
        if (out) out[n] = c->last_surface[f];
        if (frame_status) frame_status[n] = c->last_surface_status[f];
    }
    return n;
}

// ---- rule C13: principal frames and the per-cluster guess ---------------------------------------------------
int cd_shape_frame_struct_size(void) { return (int)sizeof(cd_shape_frame); }

int cd_shape_frame_host(const void* xyz, size_t stride, int n, cd_shape_frame* out) {
    if (!out || n < 0 || (n > 0 && !xyz) || stride < 12) return CD_ERR_INVALID_ARG;
    ShapeFrame rec;
    shape_frame_host(xyz, stride, n, &rec);
    std::memcpy(out, &rec, sizeof(rec));
    return rec.status;
}

int cd_shape_guess(const cd_shape_frame* cluster, const cd_shape_frame* template_, float guess[16], int32_t* flip) {
    if (!cluster || !template_ || !guess) return CD_ERR_INVALID_ARG;
    ShapeFrame cr, tr;
    std::memcpy(&cr, cluster, sizeof(cr));
    std::memcpy(&tr, template_, sizeof(tr));
    const int k = shape_guess(cr, tr, guess);
    if (flip) *flip = k;
    return CD_OK;
}

int cd_template_shape_frame(const cd_context* c, int slot, cd_shape_frame* out) {
    if (!c || !out || slot < 0 || slot >= CD_MAX_TEMPLATES) return CD_ERR_INVALID_ARG;
    if (c->tpl_m[slot] <= 0) return CD_ERR_NO_TEMPLATE;
    std::memcpy(out, &c->tpl_frame[slot], sizeof(*out));
    return CD_OK;
}

int cd_get_cluster_shape_frames(const cd_context* c, int frame, int first, int capacity, cd_shape_frame* out) {
    if (!c || frame < 0 || first < 0 || capacity < 0 || (capacity > 0 && !out)) return CD_ERR_INVALID_ARG;
    if (!c->last_shapes_ok) return CD_ERR_INVALID_ARG;   // (no fused call in CD_GUESS_CLUSTER mode since the last compute call)
    if ((size_t)frame + 1 >= c->last_first.size()) return CD_ERR_INVALID_ARG;
    const int lo = c->last_first[(size_t)frame], hi = c->last_first[(size_t)frame + 1];
    if (lo < 0 || hi < lo || (size_t)hi > c->last_shapes.size()) return CD_ERR_INVALID_ARG;
    int n = 0;
    for (int k = lo + first; k < hi && n < capacity; ++k) out[n++] = c->last_shapes[(size_t)k];
    return n;
}

static int cd_shape_frames_impl(cd_context* c, const void* xyz, size_t stride, const int32_t* offsets, int n_sets, cd_shape_frame* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!offsets || !out || n_sets <= 0 || stride < 12 || offsets[0] < 0) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    for (int i = 0; i < n_sets; ++i) if (offsets[i + 1] < offsets[i]) return fail(c, CD_ERR_INVALID_ARG, "offsets must ascend");
    const int base = offsets[0], total = offsets[n_sets] - base;
    if (total > 0 && !xyz) return fail(c, CD_ERR_INVALID_ARG, "null points");
    invalidate_last(c);
    GROW(c, d_shpts, (size_t)std::max(total, 1));
    GROW(c, d_shcl, (size_t)n_sets);
    GROW(c, d_shape, (size_t)n_sets);
    std::vector<IcpCluster> sets((size_t)n_sets);
    for (int i = 0; i < n_sets; ++i) sets[(size_t)i] = IcpCluster{offsets[i] - base, offsets[i + 1] - offsets[i], 0, i, 0, 0, 0, 0};
    int st = upload_points(c, (const char*)xyz + (size_t)base * stride, stride, total, c->d_shpts);
    if (st) return st;
    HIPCHK(c, copy_sync(c, c->d_shcl, sets.data(), sizeof(IcpCluster) * (size_t)n_sets, hipMemcpyHostToDevice));
    LAUNCH(c, launch_shape_frames(c->stream, n_sets, c->d_shcl, c->d_shpts, c->d_shape, nullptr, nullptr, nullptr));
    HIPCHK(c, copy_sync(c, out, c->d_shape, sizeof(ShapeFrame) * (size_t)n_sets, hipMemcpyDeviceToHost));
    return CD_OK;
}

// rule C9: sne's pose message -> poseMsgToEigen's rotation -> the symmetry variant that turns the most template
// faces toward the camera -> the inverse, scene -> template, rounded once to float32
int cd_surface_guess(const float Rt[16], float guess[16]) {
    if (!Rt || !guess) return CD_ERR_INVALID_ARG;
    double H[16];
    for (int i = 0; i < 16; ++i) {
        if (!std::isfinite(Rt[i])) return CD_ERR_INVALID_ARG;
        H[i] = (double)Rt[i];
    }
    double t[3], q[4];
    cd_pose_to_position_quaternion(H, t, q);   // sne.cpp:64-96 (tf::Matrix3x3::getRotation)
    const double x = q[0], y = q[1], z = q[2], w = q[3];   // (not normalised: neither tf nor Eigen does here)
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    static const double Fd[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
    int best = 0, best_score = -1;
    for (int k = 0; k < 4; ++k) {
        int score = 0;
        for (int a = 0; a < 3; ++a) {
            const double v = (R[0][a] * Fd[k][a] * t[0] + R[1][a] * Fd[k][a] * t[1]) + R[2][a] * Fd[k][a] * t[2];
            score += v > 0.0 ? 1 : 0;
        }
        if (score > best_score) { best_score = score; best = k; }
    }
    double M[3][3];
    for (int r = 0; r < 3; ++r)
        for (int a = 0; a < 3; ++a) M[r][a] = R[r][a] * Fd[best][a];
    float g[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) g[4 * i + j] = (float)M[j][i];
        g[4 * i + 3] = (float)(-((M[0][i] * t[0] + M[1][i] * t[1]) + M[2][i] * t[2]));
    }
    g[12] = 0.f; g[13] = 0.f; g[14] = 0.f; g[15] = 1.f;
    for (int i = 0; i < 16; ++i) if (!std::isfinite(g[i])) return CD_ERR_INVALID_ARG;
    std::memcpy(guess, g, sizeof(g));
    return CD_OK;
}

void cd_default_color_gate_params(cd_color_gate_params* g) {
    if (!g) return;
    std::memset(g, 0, sizeof(*g));
    g->h_lo_max = 10; g->h_hi_min = 175;   // object_detection.py:34-41: H 0..10 and 175..180
    g->s_min = 50; g->v_min = 100;         // S 50..255, V 100..255
    g->margin = 10;                        // :62
}

int cd_set_frame_bboxes(cd_context* c, const int32_t* rects, int n_frames) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (n_frames < 0 || (n_frames > 0 && !rects)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    c->frame_rects.assign(rects, rects + 4 * (size_t)n_frames);
    return CD_OK;
}

int cd_set_bbox_source(cd_context* c, int source, const cd_color_gate_params* g) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (source != CD_BBOX_PARAMS && source != CD_BBOX_PER_FRAME && source != CD_BBOX_COLOR) return fail(c, CD_ERR_INVALID_ARG, "unknown bbox source");
    cd_color_gate_params def;
    cd_default_color_gate_params(&def);
    if (!g) g = &def;
    if (int st = check_color_params(c, g)) return st;   // (the setting stays as it was)
    c->bbox_source = source;
    c->color_prm = *g;
    return CD_OK;
}

int cd_get_bbox_source(const cd_context* c, int* source) {
    if (!c || !source) return CD_ERR_INVALID_ARG;
    *source = c->bbox_source;
    return CD_OK;
}

int cd_get_frame_bboxes(const cd_context* c, int first, int capacity, cd_color_bbox* out) {
    if (!c || first < 0 || capacity < 0 || (capacity > 0 && !out)) return CD_ERR_INVALID_ARG;
    if (!c->last_bboxes_ok) return CD_ERR_INVALID_ARG;   // (the last fused call's gate took its rectangle from cd_params, or another compute call has run since)
    int n = 0;
    for (size_t f = (size_t)first; f < c->last_bboxes.size() && n < capacity; ++f, ++n) out[n] = c->last_bboxes[f];
    return n;
}

int cd_color_bbox_batch(cd_context* c, const uint8_t* rgb8, int width, int height, int n_frames, const cd_color_gate_params* g, cd_color_bbox* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_color_bbox_batch_impl(c, rgb8, width, height, n_frames, g, out, false); });
}

int cd_color_bbox_batch_device(cd_context* c, const uint8_t* d_rgb8, int width, int height, int n_frames, const cd_color_gate_params* g, cd_color_bbox* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_color_bbox_batch_impl(c, d_rgb8, width, height, n_frames, g, out, true); });
}

void cd_default_overlay_params(cd_overlay_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->P[0] = p->P[5] = (double)384.0898742675781f;                       // K[0], K[4] of the reference's README.md:78
    p->P[2] = (double)322.4656677246094f; p->P[6] = (double)240.64073181152344f;   // K[2], K[5]
    p->P[10] = 1.0;
    p->E[0] = p->E[5] = p->E[10] = p->E[15] = 1.0;
    p->dims[0] = 0.2; p->dims[1] = 0.1; p->dims[2] = 0.03;               // iterative_closest_point.launch:39-41
    p->thickness = 2;                                                    // draw_bbox.py:66
    p->rgb[0] = 0; p->rgb[1] = 255; p->rgb[2] = 0;                       // draw_bbox.py:65
}

int cd_overlay_project(const double pose[16], const cd_overlay_params* op, cd_overlay_box* out) {
    if (!pose || !out) return CD_ERR_INVALID_ARG;
    cd_overlay_params def;
    cd_default_overlay_params(&def);
    if (!op) op = &def;
    if (overlay_params_error(op)) return CD_ERR_INVALID_ARG;
    const OverlayParams kp = overlay_kernel_params(op);
    std::memset(out, 0, sizeof(*out));
    int32_t uv[16];
    for (int k = 0; k < 8; ++k) {
        float cpt[3];
        overlay_corner(pose, kp.dims, k, cpt);
        if (!overlay_pixel(kp.M, cpt, &uv[2 * k], &uv[2 * k + 1])) return CD_OK;   // skipped: the zero record
    }
    std::memcpy(out->corners, uv, sizeof(uv));
    out->drawn = 1;
    return CD_OK;
}

void cd_default_verify_params(cd_verify_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->dims[0] = 0.2; p->dims[1] = 0.1; p->dims[2] = 0.03;               // iterative_closest_point.launch:39-41
    for (auto& row : p->slot_dims) { row[0] = 0.2; row[1] = 0.1; row[2] = 0.03; }
    p->tolerance = 0.01;
    p->min_score = 0.9;
    p->min_agree = 200;                                                  // object_pose_detection.cpp:356 (the cluster minimum)
}

int cd_verify_struct_size(int which) {
    switch (which) {
        case 0: return (int)sizeof(cd_verify_params);
        case 1: return (int)sizeof(cd_verify_box);
        default: return -1;
    }
}

int cd_verify_pixel(const cd_depth_camera* cam, const double pose[16], const cd_verify_params* vp, int u, int v, uint16_t d, int32_t* cls, double* z_r) {
    if (!pose || !cls || !z_r || verify_camera_error(cam)) return CD_ERR_INVALID_ARG;
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    for (double x : vp->dims) if (!verify_dim_ok(x)) return CD_ERR_INVALID_ARG;
    if (!verify_dim_ok(vp->tolerance)) return CD_ERR_INVALID_ARG;
    VerifySetup s;
    verify_setup(pose, vp->dims, &s);
    VerifyCounts acc = {0, 0, 0, 0, 0, 0ull};
    double z = 0.0;
    *cls = verify_pixel(s, verify_kernel_camera(cam), vp->tolerance, u, v, d, &z, &acc);
    *z_r = *cls == VERIFY_MISS ? 0.0 : z;
    return CD_OK;
}

int cd_verify_box_host(const cd_depth_camera* cam, const uint16_t* depth, const double pose[16], const cd_verify_params* vp, cd_verify_box* out) {
    if (!depth || !pose || !out || verify_camera_error(cam) || cam->width < 1 || cam->height < 1) return CD_ERR_INVALID_ARG;
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    if (verify_params_error(vp)) return CD_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    VerifySetup s;
    verify_setup(pose, vp->dims, &s);
    if (!s.verified) return CD_OK;   // the zero record
    const VerifyCam kc = verify_kernel_camera(cam);
    VerifyCounts acc = {0, 0, 0, 0, 0, 0ull};
    for (int v = 0; v < cam->height; ++v)
        for (int u = 0; u < cam->width; ++u) {
            double z;
            verify_pixel(s, kc, vp->tolerance, u, v, depth[(size_t)v * (size_t)cam->width + (size_t)u], &z, &acc);
        }
    out->verified = 1;
    out->n_hit = acc.n_hit; out->n_agree = acc.n_agree; out->n_through = acc.n_through; out->n_occluded = acc.n_occluded; out->n_invalid = acc.n_invalid;
    out->agree_abs_um = (int64_t)acc.agree_abs_um;
    verify_finish(vp, out);
    return CD_OK;
}

int cd_verify_boxes_batch(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* vp, cd_verify_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_verify_boxes_batch_impl(c, cam, depth, n_frames, poses, n_boxes, boxes_per_frame, box_dims, vp, out, false); });
}
int cd_verify_boxes_batch_device(cd_context* c, const cd_depth_camera* cam, const uint16_t* d_depth, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* vp, cd_verify_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_verify_boxes_batch_impl(c, cam, d_depth, n_frames, poses, n_boxes, boxes_per_frame, box_dims, vp, out, true); });
}
int cd_verify_last_results(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int which, const cd_verify_params* vp, cd_verify_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_verify_last_results_impl(c, cam, depth, which, vp, out, false); });
}
int cd_verify_last_results_device(cd_context* c, const cd_depth_camera* cam, const uint16_t* d_depth, int which, const cd_verify_params* vp, cd_verify_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_verify_last_results_impl(c, cam, d_depth, which, vp, out, true); });
}

int cd_draw_boxes_batch(cd_context* c, uint8_t* rgb8, int width, int height, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* op, cd_overlay_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_draw_boxes_batch_impl(c, rgb8, width, height, n_frames, poses, n_boxes, boxes_per_frame, op, out, false); });
}
int cd_draw_boxes_batch_device(cd_context* c, uint8_t* d_rgb8, int width, int height, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* op, cd_overlay_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_draw_boxes_batch_impl(c, d_rgb8, width, height, n_frames, poses, n_boxes, boxes_per_frame, op, out, true); });
}
int cd_draw_last_results(cd_context* c, uint8_t* rgb8, int width, int height, int which, const cd_overlay_params* op, cd_overlay_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_draw_last_results_impl(c, rgb8, width, height, which, op, out, false); });
}
int cd_draw_last_results_device(cd_context* c, uint8_t* d_rgb8, int width, int height, int which, const cd_overlay_params* op, cd_overlay_box* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_draw_last_results_impl(c, d_rgb8, width, height, which, op, out, true); });
}

int cd_set_frame_guesses(cd_context* c, const float* guesses, int n_frames) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (n_frames < 0 || (n_frames > 0 && !guesses)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    for (size_t i = 0; i < 16 * (size_t)n_frames; ++i)
        if (!std::isfinite(guesses[i])) return fail(c, CD_ERR_INVALID_ARG, "a guess holds a non-finite value");
    c->frame_guess.assign(guesses, guesses + 16 * (size_t)n_frames);
    return CD_OK;
}

// the compute entry points proper: each call runs under the per-device scan lock (with_scan_retry)
int cd_crop_voxel(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float* out_xyz, uint32_t* out_rgb, int capacity, int* out_n_cropped, int* out_n_voxels) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_crop_voxel_impl(c, points, stride, n, p, out_xyz, out_rgb, capacity, out_n_cropped, out_n_voxels); });
}
int cd_segment_plane(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, float coeff[4], int32_t* inliers, int capacity, int* out_n_inliers, int* out_iterations) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_segment_plane_impl(c, xyz, stride, n, p, coeff, inliers, capacity, out_n_inliers, out_iterations); });
}
int cd_surface_frame(cd_context* c, const void* xyz, size_t stride, int n, const float table_normal[3], int invert, const cd_params* p, cd_surface_frame_result* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_surface_frame_impl(c, xyz, stride, n, table_normal, invert, p, out); });
}
int cd_surface_batch(cd_context* c, const void* xyz, size_t stride, int points_per_frame, const int32_t* n_points, int n_frames, const float* table_normals, int invert, const cd_params* p, cd_surface_frame_result* out, int32_t* frame_status) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_surface_batch_impl(c, xyz, stride, points_per_frame, n_points, n_frames, table_normals, invert, p, out, frame_status); });
}
int cd_bbox_filter(cd_context* c, const void* xyz, size_t stride, int n, const double P[12], const int32_t rect[4], int32_t* out_indices, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_bbox_filter_impl(c, xyz, stride, n, P, rect, out_indices, capacity, out_n); });
}
int cd_extract(cd_context* c, const void* points, size_t stride, int n, const int32_t* indices, int n_indices, int negative, void* out_points, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_extract_impl(c, points, stride, n, indices, n_indices, negative, out_points, capacity, out_n); });
}
int cd_passthrough(cd_context* c, const void* points, size_t stride, int n, int field, double limit_min, double limit_max, int negative, void* out_points, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&] { return cd_passthrough_impl(c, points, stride, n, field, limit_min, limit_max, negative, out_points, capacity, out_n); });
}
int cd_cluster(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, int32_t* labels, int32_t* sizes, int sizes_capacity, int* out_k) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_cluster_impl(c, xyz, stride, n, p, labels, sizes, sizes_capacity, out_k); });
}
int cd_icp(cd_context* c, int slot, const void* src_xyz, size_t stride, int n, const cd_params* p, cd_cluster_result* out, float* aligned) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_icp_impl(c, slot, src_xyz, stride, n, p, out, aligned); });
}
int cd_shape_frames(cd_context* c, const void* xyz, size_t stride, const int32_t* offsets, int n_sets, cd_shape_frame* out) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_shape_frames_impl(c, xyz, stride, offsets, n_sets, out); });
}
int cd_process_batch_device(cd_context* c, const void* d_frames, size_t stride, int points_per_frame, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_process_batch_device_impl(c, d_frames, stride, points_per_frame, n_frames, p, results, plane_inliers, labels); });
}
int cd_process_batch(cd_context* c, const void* frames, size_t stride, int points_per_frame, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_process_batch_impl(c, frames, stride, points_per_frame, n_frames, p, results, plane_inliers, labels); });
}
int cd_ground_plane(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float coeff[4], void* out_records, int capacity, int* out_n, int* out_n_inliers) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_ground_plane_impl(c, points, stride, n, p, coeff, out_records, capacity, out_n, out_n_inliers); });
}
int cd_depth_to_cloud(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, void* out_records, size_t stride, int rgb_offset, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_depth_to_cloud_impl(c, cam, depth, color, out_records, stride, rgb_offset, capacity, out_n); });
}
int cd_process_depth_batch(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_process_depth_batch_impl(c, cam, depth, color, n_frames, p, results, plane_inliers, labels, false); });
}
int cd_depth_to_cloud_mapped(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* depth, const uint8_t* color, void* out_records, size_t stride, int rgb_offset, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_depth_to_cloud_impl(c, cam, depth, color, out_records, stride, rgb_offset, capacity, out_n, ccam, true); });
}
int cd_process_depth_batch_mapped(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* depth, const uint8_t* color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_process_depth_batch_impl(c, cam, depth, color, n_frames, p, results, plane_inliers, labels, false, ccam, true); });
}
int cd_process_depth_batch_mapped_device(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* d_depth, const uint8_t* d_color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_process_depth_batch_impl(c, cam, d_depth, d_color, n_frames, p, results, plane_inliers, labels, true, ccam, true); });
}
int cd_process_depth_batch_device(cd_context* c, const cd_depth_camera* cam, const uint16_t* d_depth, const uint8_t* d_color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!c) return CD_ERR_INVALID_ARG;
    return with_scan_retry(c, [&]() { return cd_process_depth_batch_impl(c, cam, d_depth, d_color, n_frames, p, results, plane_inliers, labels, true); });
}

int cd_get_timing(const cd_context* c, cd_timing* out) {
    if (!c || !out) return CD_ERR_INVALID_ARG;
    *out = c->timing;
    return CD_OK;
}

void cd_pose_to_position_quaternion(const double H[16], double pos[3], double q[4]) {
    pos[0] = H[3]; pos[1] = H[7]; pos[2] = H[11];
    const double m[3][3] = {{H[0], H[1], H[2]}, {H[4], H[5], H[6]}, {H[8], H[9], H[10]}};
    const double trace = m[0][0] + m[1][1] + m[2][2];
    double t[4];
    if (trace > 0.0) {
        double s = std::sqrt(trace + 1.0);
        t[3] = s * 0.5;
        s = 0.5 / s;
        t[0] = (m[2][1] - m[1][2]) * s;
        t[1] = (m[0][2] - m[2][0]) * s;
        t[2] = (m[1][0] - m[0][1]) * s;
    } else {
        const int i = m[0][0] < m[1][1] ? (m[1][1] < m[2][2] ? 2 : 1) : (m[0][0] < m[2][2] ? 2 : 0);
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double s = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        t[i] = s * 0.5;
        s = 0.5 / s;
        t[3] = (m[k][j] - m[j][k]) * s;
        t[j] = (m[j][i] + m[i][j]) * s;
        t[k] = (m[k][i] + m[i][k]) * s;
    }
    q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; q[3] = t[3];
}

void cd_bbox_corners(const double H[16], double l, double w, double h, float out[24]) {
    float Hf[16];
    for (int i = 0; i < 16; ++i) Hf[i] = (float)H[i];
    const double sx[8] = {-1, -1, -1, -1, 1, 1, 1, 1}, sy[8] = {-1, -1, 1, 1, -1, -1, 1, 1}, sz[8] = {-1, 1, -1, 1, -1, 1, -1, 1};
    for (int k = 0; k < 8; ++k) {
        const float x = (float)(sx[k] * l / 2), y = (float)(sy[k] * w / 2), z = (float)(sz[k] * h / 2);
        out[3 * k] = ((Hf[0] * x + Hf[1] * y) + Hf[2] * z) + Hf[3];
        out[3 * k + 1] = ((Hf[4] * x + Hf[5] * y) + Hf[6] * z) + Hf[7];
        out[3 * k + 2] = ((Hf[8] * x + Hf[9] * y) + Hf[10] * z) + Hf[11];
    }
}

}  // extern "C"
