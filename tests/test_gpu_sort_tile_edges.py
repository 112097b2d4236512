"""The voxel sort at the boundaries of its tiles.  k_radix_scatter works on tiles of 4096 (run or point) records, k_voxel_runs and
k_radix_ghist on tiles of 8192; the clouds here put EVERY kept point into a cell of its own (lattice points two leaves apart, in
a shuffled order), so that a frame of n points is n runs, n sort elements and n voxels, and n can be set to one below, on and one
above a multiple of either tile size.  Each case is compared with the oracle the way test_voxel_stage_by_runs_and_by_points does:
counts and voxel cloud bits (points and colours), through every path of the voxel stage."""
import numpy as np
import pytest

from perception_amd import capi

LEAF = 0.005                       # the default leaf: cells (cx, cy, cz) = floor(p / LEAF)
NX, NZ, NY = 40, 89, 4             # lattice sites inside the default crop (x in +-0.2, z in 0..0.9), two cells apart on every axis
MAX_POINTS = 20000
COUNTS = (1, 4095, 4096, 4097, 8191, 8192, 8193, 12289)


def _records(cells, rng):
    """One record x y z rgb at the centre of each cell (cx, cy, cz), in the order given."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    rec = np.zeros((len(cells), 4), np.float32)
    rec[:, :3] = (cells + 0.5) * LEAF
    rec[:, 3] = rng.randint(0, 1 << 24, len(cells)).astype(np.uint32).view(np.float32)
    return rec


def _lattice(n, rng):
    """n distinct sites of the NX x NY x NZ lattice in a random order: no two points share a cell, whatever their order."""
    site = rng.permutation(NX * NY * NZ)[:n]
    assert len(site) == n
    i, j, k = site % NX, (site // NX) % NY, site // (NX * NY)
    return _records(np.stack([-39 + 2 * i, 2 * j, 1 + 2 * k], 1), rng)


def _pad(rec, n):
    """the frame as n records: NaN points (which the crop drops) behind the real ones"""
    out = np.full((n, 4), np.nan, np.float32)
    out[:len(rec)] = rec
    return out


@pytest.fixture(scope="module")
def cases(O):
    """name -> (records, oracle points, oracle colours): computed once, not modified afterwards.  The oracle alone confirms what
    the clouds are built for: every point is kept and is a voxel of its own."""
    rng = np.random.RandomState(4096)
    prm = capi.default_params()
    prm.rgb_offset = 12
    clouds = {"n%d" % n: _lattice(n, rng) for n in COUNTS}
    # keys that differ in their lowest digit only: one row of cells along x (the packed key's lowest field; voxel index i)
    clouds["one_digit"] = _records([(-39 + 2 * i, 0, 41) for i in rng.permutation(NX)], rng)
    # every run in ONE bin of the lowest digit of the packed key (x cell and the parity of the y cell fixed) while the upper
    # digits vary, over more than one scatter tile: 51 x 89 = 4539 cells
    yz = [(1, 2 * j, 1 + 2 * k) for j in range(-25, 26) for k in range(NZ)]
    clouds["one_low_bin"] = _records([yz[q] for q in rng.permutation(len(yz))], rng)
    clouds["empty"] = np.zeros((0, 4), np.float32)
    clouds["n5000"] = _lattice(5000, rng)
    clouds["n300"] = _lattice(300, rng)
    out = {}
    for name, rec in clouds.items():
        n = len(rec)
        if n == 0:
            out[name] = (rec, np.zeros((0, 3), np.float32), np.zeros(0, np.uint32))
            continue
        st, vo, ro, nco, _ = O.crop_voxel(rec, prm, want_rgb=True)
        assert st == capi.CD_OK and nco == n and len(vo) == n, (name, st, nco, len(vo))
        out[name] = (rec, vo, ro)
    return out


def test_every_point_is_its_own_voxel(cases):
    """(CPU) the property the GPU cases rest on, by the oracle alone - asserted while the fixture is built; here: the case list"""
    assert {"n%d" % n for n in COUNTS} <= set(cases) and len(cases["one_low_bin"][0]) > 4096 and len(cases["one_digit"][0]) == NX


BATCHES = (("n5000", "empty", "n300"), ("n4097", "n12289", "n1"))   # an empty frame inside a batch; three different counts


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["crop_runs", "runs", "points", "wide32"])
def test_sort_tile_edges(O, cases, template, path, monkeypatch):
    """crop_runs: the default (k_crop_runs' records, scatters only); runs: CUBOID_CROP_RUNS=0 (k_voxel_runs, then the scatters);
    points: CUBOID_VOXEL_RUNS=0 (k_radix_ghist, the scatters move points); wide32: 32-byte records, which take the copying crop."""
    if path == "runs":
        monkeypatch.setenv("CUBOID_CROP_RUNS", "0")
    if path == "points":
        monkeypatch.setenv("CUBOID_VOXEL_RUNS", "0")
    wide = path == "wide32"
    prm = capi.default_params()
    prm.rgb_offset = 16 if wide else 12

    def layout(rec):
        if not wide:
            return rec
        w = np.zeros((len(rec), 8), np.float32)
        w[:, :3] = rec[:, :3]
        w[:, 4] = rec[:, 3]
        return w

    cx = capi.Context(max_points=MAX_POINTS, max_frames=3)
    try:
        for name, (rec, vo, ro) in cases.items():
            if len(rec) == 0:
                continue
            vox, rgb, nc = cx.crop_voxel(layout(rec), prm, want_rgb=True)
            assert nc == len(rec) and len(vox) == len(vo), (name, nc, len(vox))
            assert np.array_equal(vox.view(np.uint32), vo.view(np.uint32)) and np.array_equal(rgb, ro), name
        # frames of a batch: the tickets of the sort's tiles are drawn per frame, and the frames' tile counts differ
        cx.set_template(0, template)
        bp = capi.default_params()
        bp.rgb_offset = prm.rgb_offset
        bp.plane_max_iterations = 10      # (the stages behind the voxel grid run too: keep them short)
        bp.cluster_enable = 0
        bp.icp_max_iterations = 1
        for names in BATCHES:
            npts = max(len(cases[nm][0]) for nm in names)
            batch = np.stack([layout(_pad(cases[nm][0], npts)) for nm in names], 0)
            res, _, _ = cx.process_batch(batch, bp)
            for f, nm in enumerate(names):
                rec, vo, ro = cases[nm]
                assert res[f].n_cropped == len(rec) and res[f].n_voxels == len(vo), (names, f)
                if len(rec) == 0:
                    continue
                got = cx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, 12)
                assert np.array_equal(got[:, :3], vo.view(np.uint32)) and np.array_equal(got[:, 3], ro), (names, f)
    finally:
        cx.close()
