// tunables.hpp - what the CUBOID_* environment variables set.  Plain data, no HIP: the context holds one (context.hpp) and the
// host-only ICP planner reads it (icp_plan.hpp).
#pragma once

// Read once per context (read_tunables, context.hip).  CUBOID_DEBUG, CUBOID_ICP_GRID_RC and CUBOID_ICP_CELL_FACTOR are read
// where they are used.
struct Tunables {
    bool crop_two_pass = false;   // CUBOID_CROP_TWO_PASS=1: always the two-pass crop
    int icp_persist = 1;          // CUBOID_ICP_PERSIST=0: the sliced driver always in its multi-launch form; 2: the persistent
                                  // launch starts with its abort flag raised (tests the hand-over to the multi-launch form)
    bool crop_runs = true;        // CUBOID_CROP_RUNS=0: the crop writes per-point keys and k_voxel_runs finds the runs (rounds 2-3)
    int don_idle = 0, don_fault = 0;   // CUBOID_ICP_DON_IDLE / CUBOID_ICP_DON_FAULT: tests of the hand-over path (IcpParams::don_idle / don_fault)
    int icp_donate = -1;          // CUBOID_ICP_DONATE: -1 auto (a call alone on the device), 0 never, 1 always
    int force_stall = 0;          // CUBOID_FORCE_SCAN_STALL=n: the next n chained-scan checks report a stall (tests the retry)
    int icp_mode = 0;             // CUBOID_ICP_MODE: 0 auto, 1 sliced multi-launch, 2 whole-cluster kernel, 3 grouped pipe
    int icp_max_wg = 0;           // > 0: cap on the persistent ICP grid (CUBOID_ICP_MAX_WG; tests force slot refills with it)
    int icp_cpw = 0;              // CUBOID_ICP_CPW: clusters per workgroup a persistent ICP launch is sized for (0: by regime, whole_launch_grid)
    int icp_direct = 1;           // CUBOID_ICP_DIRECT=0: an all-lattice ICP stage uploads its lists and reads its results back by copy launches
    int mirror_reads = 1;         // CUBOID_MIRROR_READS=0: active flags and chosen plane models are uploaded before the kernels that read them
    int mirror_writes = 1;        // CUBOID_MIRROR_WRITES=0: every host read-back of the FrameState array is a copy launch again
    int cluster_cells = 1;        // CUBOID_CLUSTER_CELLS=0: frames above 8192 object points straight to the point-graph kernels (rounds 1-5)
    int cluster_tiers = 1;        // CUBOID_CLUSTER_TIERS=0: k_cluster_lds (150 KiB of LDS, 1024 threads) for every frame up to 8192 object points, and
                                  // the 64 KiB sampler map for every RANSAC round, as before the small tiers
    int crop_direct = 1;          // CUBOID_CROP_DIRECT=0: the crop always copies the kept points (rounds 1-5)
    int centroid_lanes = 1;       // CUBOID_CENTROID_LANES=0: the quad-per-voxel centroid kernel (rounds 3-5) instead of a lane per voxel
    bool voxel_runs = true;       // CUBOID_VOXEL_RUNS=0: S1 sorts the cropped points instead of their runs of equal voxel index
    int icp_slots = 0;            // CUBOID_ICP_SLOTS: clusters in flight per workgroup, 1 .. CD_PIPE_SLOTS (0: by regime)
    int icp_big_weight = 0;       // workgroup share of a template in global memory, per point (CUBOID_ICP_BIG_WEIGHT; 0 = by the launch's regime, measured on config 5)
    int icp_lattice = 1;          // CUBOID_ICP_LATTICE=0: lattice templates take the generic searches too (A/B, fallback tests)
    int zero_once = 1;            // CUBOID_ZERO_ONCE=0: every stage of a fused batch call fills its scratch arrays itself (A/B)
    int copy_kernels = 1;         // CUBOID_COPY_KERNELS=0: the small pinned <-> device transfers go through hipMemcpyAsync (SDMA) again
    int lat_shape[3] = {0, 0, 0};   // CUBOID_LAT_SHAPE=cpw,wpc[,per_slot]: clusters per workgroup, waves per cluster, clusters per slot of k_icp_lat (0: by regime)
    int front_concurrent = 0;     // CUBOID_FRONT_CONCURRENT: at most that many fused batch calls of the device between crop and clusters (0 = no gate)
    int icp_concurrent = 0;       // CUBOID_ICP_CONCURRENT: admission gate of the whole-cluster ICP launches (0 = none)
    int icp_lowprio = 1;          // CUBOID_ICP_LOWPRIO: 0 never, 1 the launches of a mixed-template batch (measured: config 5 +30 %), 2 every
                                  // persistent ICP launch (config 3: -1 %)
};
