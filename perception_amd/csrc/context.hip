// context.hip - the context (cd_create / cd_destroy), what the contexts of a device share, the copy and buffer helpers of
// every unit, and the small host-side entries of include/cuboid_hip.h: defaults, struct sizes, setters and getters.
// The whole chain runs on one HIP stream with every intermediate resident in HBM (frame-major arrays, pitch = points per
// frame).  The host only (a) sizes launches from a handful of per-frame scalars mirrored through pinned memory, (b) replays
// PCL's sequential RANSAC stop rule over the batched inlier counts, (c) solves the 3x3 plane-refit eigenproblem and (d) polls
// ICP completion.  There is no CPU compute fallback of any stage.
#include <random>

#include "context.hpp"

namespace cd {
static DeviceShared g_shared[MAX_DEVICES];   // the only instance
DeviceShared& device_shared(const cd_context* c) { return g_shared[c->device & (MAX_DEVICES - 1)]; }

// blocking copy ordered on the context's own (non-blocking) stream: the NULL stream gives no ordering against it
hipError_t copy_sync(cd_context* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}

// a small transfer between a PINNED host mirror of the context and device memory, as a kernel on the context's stream
// (launch_copy_rows, k_plane.hip: why not hipMemcpyAsync).  bytes: a multiple of 4.  CUBOID_COPY_KERNELS=0: hipMemcpyAsync (A/B).
hipError_t xfer(cd_context* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!c->tun.copy_kernels || (bytes & 3)) return hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    launch_copy_rows(c->stream, dst, bytes, src, bytes, bytes, 1);
    return hipGetLastError();
}

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

int sync_fs(cd_context* c, int F, bool copied) {
    if (!copied) HIPCHK(c, xfer(c, c->h_fs, c->d_fs, sizeof(FrameState) * F, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < F; ++f)
        if (c->h_fs[f].scan_stalled) return fail(c, CD_INTERNAL_STALL, "a chained scan stalled (workgroups of a grid were not started in id order)");
    if (c->tun.force_stall > 0) { c->tun.force_stall -= 1; return fail(c, CD_INTERNAL_STALL, "a chained scan stalled (forced: CUBOID_FORCE_SCAN_STALL)"); }
    return CD_OK;
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

// float4 points on the device -> `m` records of `stride` bytes in caller memory (k_pack_records, then ONE download).
// The staging area is the context's input buffer (its contents - the frames of a host-pointer call - are dead by now).
int download_records(cd_context* c, const float4* d_pts, int m, size_t stride, int rgb_offset, uint32_t pad3, void* out, size_t staging_skip) {
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
}  // namespace cd

// every CUBOID_* switch a context mirrors, read when the context is created (before its streams: icp_lowprio sets their priority)
static void read_tunables(Tunables* t) {
    auto num = [](const char* name, int* v) { if (const char* m = std::getenv(name)) *v = std::atoi(m); };
    auto count = [](const char* name, int* v) { if (const char* m = std::getenv(name)) *v = std::max(0, std::atoi(m)); };
    auto flag = [](const char* name, auto* v) { if (const char* m = std::getenv(name)) *v = std::atoi(m) != 0; };
    num("CUBOID_ICP_LOWPRIO", &t->icp_lowprio);
    count("CUBOID_ICP_MAX_WG", &t->icp_max_wg);
    count("CUBOID_ICP_CPW", &t->icp_cpw);
    count("CUBOID_ICP_SLOTS", &t->icp_slots);
    num("CUBOID_ICP_DONATE", &t->icp_donate);
    count("CUBOID_ICP_DON_IDLE", &t->don_idle);
    num("CUBOID_ICP_DON_FAULT", &t->don_fault);
    num("CUBOID_ICP_LATTICE", &t->icp_lattice);
    num("CUBOID_COPY_KERNELS", &t->copy_kernels);
    num("CUBOID_ZERO_ONCE", &t->zero_once);
    if (const char* m = std::getenv("CUBOID_LAT_SHAPE")) std::sscanf(m, "%d,%d,%d", &t->lat_shape[0], &t->lat_shape[1], &t->lat_shape[2]);
    flag("CUBOID_VOXEL_RUNS", &t->voxel_runs);
    flag("CUBOID_CENTROID_LANES", &t->centroid_lanes);
    flag("CUBOID_CROP_DIRECT", &t->crop_direct);
    flag("CUBOID_CLUSTER_CELLS", &t->cluster_cells);
    flag("CUBOID_CLUSTER_TIERS", &t->cluster_tiers);
    flag("CUBOID_MIRROR_WRITES", &t->mirror_writes);
    flag("CUBOID_MIRROR_READS", &t->mirror_reads);
    flag("CUBOID_ICP_DIRECT", &t->icp_direct);
    count("CUBOID_ICP_BIG_WEIGHT", &t->icp_big_weight);
    flag("CUBOID_CROP_TWO_PASS", &t->crop_two_pass);
    num("CUBOID_ICP_PERSIST", &t->icp_persist);
    count("CUBOID_FORCE_SCAN_STALL", &t->force_stall);
    flag("CUBOID_CROP_RUNS", &t->crop_runs);
    count("CUBOID_ICP_CONCURRENT", &t->icp_concurrent);
    count("CUBOID_FRONT_CONCURRENT", &t->front_concurrent);
    if (const char* m = std::getenv("CUBOID_ICP_MODE")) t->icp_mode = !std::strcmp(m, "sliced") ? 1 : (!std::strcmp(m, "cluster") ? 2 : (!std::strcmp(m, "pipe") ? 3 : 0));
}

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
    read_tunables(&c->tun);
    // non-blocking: no implicit ordering against the NULL stream (torch ops, other contexts in flight)
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
        const int prio = c->tun.icp_lowprio ? prio_least : 0;
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

int cd_set_frame_guesses(cd_context* c, const float* guesses, int n_frames) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (n_frames < 0 || (n_frames > 0 && !guesses)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    for (size_t i = 0; i < 16 * (size_t)n_frames; ++i)
        if (!std::isfinite(guesses[i])) return fail(c, CD_ERR_INVALID_ARG, "a guess holds a non-finite value");
    c->frame_guess.assign(guesses, guesses + 16 * (size_t)n_frames);
    return CD_OK;
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
