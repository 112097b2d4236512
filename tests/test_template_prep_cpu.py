"""Template preparation on the CPU (no GPU): perception_amd/csrc/template_prep.hpp through its stand-alone program
template_prep_check.  Every input must satisfy the invariants the ICP search kernels rely on (--check) and give, byte for byte,
the layouts recorded in template_prep_digests.json - FNV-1a digests of everything cd_set_template uploads, recorded from the
commit BEFORE the preparation moved into that header (it was a static function of cuboid_hip.hip then).  The file is data: a
digest that differs means the preparation changed what the kernels get."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from perception_amd import pcd, synth, templates

F32 = np.float32
CSRC = os.path.join(ROOT, "perception_amd", "csrc")
EXE = os.path.join(CSRC, "template_prep_check")
with open(os.path.join(ROOT, "tests", "template_prep_digests.json")) as _f:
    DIGESTS = json.load(_f)


def _random(m, seed=None):
    return np.random.default_rng(m if seed is None else seed).uniform(-0.1, 0.1, (m, 3)).astype(F32)


def _coplanar():
    xx, yy = np.meshgrid(np.arange(25) * 0.004, np.arange(20) * 0.004)
    return np.stack([xx.ravel(), yy.ravel(), np.full(500, 0.5)], 1).astype(F32)


def _with_infinities():
    a = _random(200, seed=1001)
    a[17, 0], a[120, 2] = np.inf, -np.inf
    return a


def _golden(name):
    return lambda: pcd.read_xyz(os.path.join(GOLDEN, name)).astype(F32)


CASES = {"random_%d" % m: (lambda m=m: _random(m)) for m in (
    1, 2, 63, 64, 65, 129, 200,          # the pad and the first split
    7552, 7553, 9000,                    # across ICP_TPL_LDS: chunk and superpatch tables appear, big_ok turns on
    65535, 65536, 70000)}                # across ICP_BIG_MAX: kdmap / cell_start / big_ok turn off
CASES.update({
    "identical_100": lambda: np.tile(_random(1, seed=1000), (100, 1)),   # no positive neighbour distance: the pitch fallback
    "coplanar_25x20": _coplanar,
    "infinities_200": _with_infinities,
    "default_cuboid": lambda: templates.template_xyz32(**templates.DEFAULT_TEMPLATE),
    "cuboid_L200_W100_H75_6faces": _golden("template_cuboid_L200_W100_H75.pcd"),
    "cuboid_L200_W100_H75_3faces": _golden("template_cuboid_L200_W100_H75_3faces.pcd"),
    "cuboid_L200_W75_H100_3faces": _golden("template_cuboid_L200_W75_H100_3faces.pcd")})
CASES.update({"config5_%d" % k: (lambda d=d: templates.template_xyz32(*d)) for k, d in enumerate(synth.CONFIG5_DIMS)})
CASES.update({name: _golden(name + "_ascii.pcd") for name in ("clamp", "eraser", "marker", "screwdriver")})


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-C", CSRC, "template_prep_check"], check=True, stdout=subprocess.DEVNULL)
    return EXE


def _run(exe, tmp_path, xyz, *flags):
    assert xyz.dtype == F32 and xyz.ndim == 2 and xyz.shape[1] == 3
    path = os.path.join(str(tmp_path), "points.bin")
    xyz.astype("<f4").tofile(path)
    return subprocess.run([exe, *flags, path], capture_output=True, text=True, timeout=120)


def test_every_case_has_a_recorded_digest():
    assert sorted(CASES) == sorted(DIGESTS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants_hold_and_layout_is_the_recorded_one(exe, tmp_path, name):
    r = _run(exe, tmp_path, CASES[name](), "--check")
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == DIGESTS[name]


def test_nan_coordinate_is_survived(exe, tmp_path):
    """Not digested, and not --check'ed: the k-d comparator (key, then original index) is no strict weak ordering once a key is
    NaN, so what std::nth_element leaves then depends on the C++ library.  What must hold: the preparation ends, the template is
    no lattice and its principal frame is refused for its coordinates."""
    a = _random(200, seed=1002)
    a[77, 1] = np.nan
    r = _run(exe, tmp_path, a)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split())
    assert fields["m"] == "200" and fields["nface"] == "0"
    assert int(fields["frame_status"]) == -1      # SHAPE_ERR_INVALID = CD_ERR_INVALID_ARG
