"""Rule C15 (point labels) without a GPU: the names the header and capi.py export, the numpy restatement
(perception_amd/point_labels.py) against the oracle's records, the host check of label_math.hpp, the tint."""
import os
import re
import subprocess

import numpy as np
import pytest

from perception_amd import capi, point_labels as PL, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_label_points_last", "cd_label_points_last_device", "cd_label_depth_last", "cd_label_depth_last_device",
               "cd_default_label_palette", "cd_label_struct_size", "cd_tint_labels_batch", "cd_tint_labels_batch_device"]


def test_header_and_capi_export_the_label_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS, name
    m = re.search(r"enum\s*\{\s*CD_LABEL_INVALID = (\d+), CD_LABEL_CROPPED = (\d+), CD_LABEL_PLANE = (\d+), CD_LABEL_OBJECT = (\d+), "
                  r"CD_LABEL_GATED = (\d+), CD_LABEL_CLUSTER0 = (\d+)\s*\}", header)
    assert m and [int(v) for v in m.groups()] == [0, 1, 2, 3, 4, 8]
    assert (capi.CD_LABEL_INVALID, capi.CD_LABEL_CROPPED, capi.CD_LABEL_PLANE, capi.CD_LABEL_OBJECT, capi.CD_LABEL_GATED,
            capi.CD_LABEL_CLUSTER0) == (0, 1, 2, 3, 4, 8)
    assert (PL.LABEL_INVALID, PL.LABEL_CROPPED, PL.LABEL_PLANE, PL.LABEL_OBJECT, PL.LABEL_GATED, PL.LABEL_CLUSTER0) == (0, 1, 2, 3, 4, 8)
    try:
        lib = capi.load_library()
    except OSError:
        lib = None
    import ctypes
    if lib is not None:
        assert lib.cd_label_struct_size(0) == ctypes.sizeof(capi.CdLabelPalette) == 1024 and lib.cd_label_struct_size(1) == -1
        assert np.array_equal(capi.default_label_palette(), PL.default_palette())
    else:
        assert re.search(r"typedef struct cd_label_palette \{ uint8_t rgba\[256\]\[4\]; \} cd_label_palette;", header)
        assert ctypes.sizeof(capi.CdLabelPalette) == 1024


def _identities(O, frame, prm, template):
    """The oracle's records of the frame, its labels by the numpy rule, and the count identities every case shares."""
    o = O.process_frame(frame, prm, template, want_clouds=True, all_clusters=64)
    r = o["result"]
    lab = PL.labels_of_frame(frame, prm, r.n_voxels, o["plane_inliers"], o["voxels"], o["objects"], o["labels"])   # (asserts the cell count)
    assert lab.dtype == np.uint8 and lab.shape == (len(frame),)
    assert int((lab >= 2).sum()) == r.n_cropped
    assert not np.isin(lab, (5, 6, 7)).any()
    fin = np.isfinite(frame[:, :3]).all(1)
    assert np.array_equal(lab == 0, ~fin)
    cls = PL.voxel_classes(r.n_voxels, o["plane_inliers"], o["voxels"], o["objects"], o["labels"]) if r.n_voxels else np.zeros(0, np.uint8)
    in_both = len(np.intersect1d(o["plane_inliers"], PL.object_voxels(o["voxels"], o["objects"]))) if r.n_voxels else 0
    assert int((cls == 2).sum()) == r.n_plane - in_both
    assert int(np.isin(cls, (2, 4)).sum()) == r.n_voxels - r.n_objects
    sizes = [c.size for c in o["clusters"]]
    assert len(sizes) == r.n_clusters
    for k, size in enumerate(sizes[:248]):
        assert int((cls == 8 + k).sum()) == size, k
    # every point takes the class of a voxel: no class without a point, no point label that no voxel has
    assert set(np.unique(lab[lab >= 2])) == set(np.unique(cls))
    return o, lab, cls


CASES = [(96, 72, 2, [466]), (160, 120, 0, [499]), (160, 120, 3, [859, 506]), (200, 150, 1, [989, 702]), (640, 480, 5, None)]


@pytest.mark.parametrize("w,h,idx,sizes", CASES)
def test_numpy_rule_against_the_oracle(O, template, w, h, idx, sizes):
    prm = capi.default_params()
    frame = synth.frame(idx, width=w, height=h)
    o, lab, cls = _identities(O, frame, prm, template)
    r = o["result"]
    assert int((cls == 2).sum()) == r.n_plane          # extract_negative = 1: no inlier is an object
    if sizes is None:
        assert r.n_clusters == 3
    else:
        assert [c.size for c in o["clusters"]] == sizes
    assert (lab == 2).any() and (lab == 8).any() and (lab == 1).any() and (lab == 0).any()


@pytest.fixture(scope="module")
def base(O, template):
    frame = synth.frame(3, width=160, height=120)
    o = O.process_frame(frame, capi.default_params(), template, want_clouds=True)
    return frame, o


def test_second_crop_through_an_object_gives_gated(O, template, base):
    frame, o = base
    prm = capi.default_params()
    prm.crop2_z_max = float(np.median(o["objects"][:, 2]))      # cuts through the object cloud
    o2, lab, cls = _identities(O, frame, prm, template)
    assert 0 < o2["result"].n_objects < o["result"].n_objects
    assert (lab == 4).any() and (cls == 4).sum() == o2["result"].n_voxels - o2["result"].n_plane - o2["result"].n_objects


def test_extract_positive(O, template, base):
    frame, _ = base
    prm = capi.default_params()
    prm.extract_negative = 0                                     # the object cloud is the plane; every non-inlier is gated
    o2, lab, cls = _identities(O, frame, prm, template)
    assert (cls == 2).sum() <= o2["result"].n_plane and (lab == 4).any()


def test_clustering_disabled_gives_rank_zero(O, template, base):
    frame, _ = base
    prm = capi.default_params()
    prm.cluster_enable = 0
    o2, lab, cls = _identities(O, frame, prm, template)
    assert set(np.unique(cls)) <= {2, 4, 8} and (cls == 8).sum() == o2["result"].n_objects


def test_min_size_above_the_largest_cluster_gives_object(O, template, base):
    frame, _ = base
    prm = capi.default_params()
    prm.cluster_min_size = 5000
    o2, lab, cls = _identities(O, frame, prm, template)
    assert o2["result"].n_clusters == 0 and (cls == 3).sum() == o2["result"].n_objects > 0 and (lab == 3).any() and not (lab >= 8).any()


def test_all_nan_frame(O, template):
    frame = np.full((500, 4), np.nan, np.float32)
    o, lab, cls = _identities(O, frame, capi.default_params(), template)
    assert o["result"].n_voxels == 0 and not lab.any()


def test_frame_without_a_plane_model_is_labelled_from_its_object_cloud(O, template):
    # two voxels: no sample of three points, no model; S3 then moves every voxel to the object cloud
    frame = np.zeros((40, 4), np.float32)
    frame[:20, :3] = [0.1005, 0.0005, 0.5005]
    frame[20:, :3] = [-0.0995, 0.0205, 0.6005]
    frame[:, :3] += np.random.default_rng(15).uniform(0, 0.004, (40, 3)).astype(np.float32)
    frame[5] = np.nan
    frame[6, 2] = 2.0
    prm = capi.default_params()
    o, lab, cls = _identities(O, frame, prm, template)
    r = o["result"]
    assert r.status == capi.CD_ERR_NO_MODEL and r.n_plane == 0
    assert r.n_objects == r.n_voxels > 0 and set(np.unique(cls)) == {3}       # every voxel is an object in no kept cluster
    assert lab[5] == 0 and lab[6] == 1 and (np.delete(lab, [5, 6]) == 3).all()


@pytest.mark.parametrize("extra", ["", "-fsanitize=address,undefined"])
def test_label_math_on_the_host(extra, tmp_path):
    """label_math_check: the key arithmetic, the search and the classes of label_math.hpp against a plain double loop."""
    exe = str(tmp_path / "label_math_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([extra] if extra else []) + [os.path.join(CSRC, "label_math_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe, "120"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ok, grids, probes, hits, outside = r.stdout.split()
    assert ok == "ok" and int(grids) == 120 and int(hits) > 10000 and int(outside) > 10000


def test_tint_by_hand():
    pal = np.zeros((256, 4), np.uint8)
    pal[2] = (128, 128, 128, 96)
    pal[4] = (139, 0, 0, 255)
    pal[8] = (230, 25, 75, 160)
    pal[255] = (0, 0, 0, 1)
    rgb = np.array([[[0, 0, 0], [255, 255, 255], [10, 20, 30], [200, 100, 50]],
                    [[7, 7, 7], [255, 0, 128], [1, 2, 3], [254, 255, 0]]], np.uint8)
    lab = np.array([[0, 2, 2, 8], [1, 4, 8, 255]], np.uint8)
    want = np.array([[[0, 0, 0],                                    # alpha 0
                      [207, 207, 207],                               # (255 * 159 + 128 * 96 + 127) / 255 = 52960 / 255
                      [54, 61, 67],                                  # (10 * 159 + 12288 + 127) / 255 = 14005 / 255, 15595 / 255, 17185 / 255
                      [219, 53, 66]],                                # (200 * 95 + 230 * 160 + 127) / 255 = 55927 / 255, 13627 / 255, 16877 / 255
                     [[7, 7, 7],
                      [139, 0, 0],                                   # alpha 255: the palette colour
                      [145, 16, 48],                                 # (95 + 36800 + 127) / 255, (190 + 4000 + 127) / 255, (285 + 12000 + 127) / 255
                      [253, 254, 0]]], np.uint8)                     # (254 * 254 + 127) / 255 = 64643 / 255, (255 * 254 + 127) / 255, 127 / 255
    assert np.array_equal(PL.tint(rgb, lab, pal), want)
    assert np.array_equal(PL.tint(rgb, lab, np.zeros((256, 4), np.uint8)), rgb)
    d = PL.default_palette()
    assert d[0, 3] == d[1, 3] == 0 and not d[5:8].any() and d[2, 0] == d[2, 1] == d[2, 2] and np.array_equal(d[8], d[16]) and not np.array_equal(d[8], d[9])
