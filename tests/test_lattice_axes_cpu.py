"""cd_lattice_axes (host only): which lattice templates have at most one face per constant axis and so take the mask-free
face code of k_icp_lat (IcpLattice::axes_distinct: lattice_classify_axes in common.hpp, called at the end of lattice_detect in
template_prep.hpp)."""
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from perception_amd import capi, pcd, synth, templates

F32 = np.float32
TABS = {0: np.arange(-1.0, 1.01, 0.25), 1: np.arange(-1.0, 1.01, 0.5), 2: np.arange(0.0, 0.51, 0.125)}   # 9 / 5 / 5 entries, exact in float32
CONST = {0: -1.25, 1: -1.5, 2: -0.125}


def lattice(faces, tabs=TABS):
    """faces: [(constant axis, fast axis, constant)] -> (M, 3) float32, each face first-axis-fastest, faces one after the other."""
    out = []
    for w, u, c in faces:
        v = 3 - w - u
        uu, vv = np.meshgrid(tabs[u], tabs[v])
        p = np.empty((uu.size, 3))
        p[:, u] = uu.ravel(); p[:, v] = vv.ravel(); p[:, w] = c
        out.append(p)
    return np.concatenate(out, 0).astype(F32)


def _face(w, fast_low=True):
    u = min(a for a in range(3) if a != w) if fast_low else max(a for a in range(3) if a != w)
    return (w, u, CONST[w])


@pytest.mark.parametrize("order", list(itertools.permutations(range(3))))
def test_three_faces_on_three_axes_in_every_order(order):
    P = lattice([_face(w, fast_low=(k != 1)) for k, w in enumerate(order)])
    assert len(capi.lattice_detect(P)) == 3
    distinct, face, c = capi.lattice_axes(P)
    assert distinct == 1
    assert face == [order.index(a) for a in range(3)]
    assert c.tolist() == [F32(CONST[a]) for a in range(3)]


@pytest.mark.parametrize("axes", [(2,), (0,), (2, 0), (1, 2), (0, 1)])
def test_one_and_two_faces(axes):
    P = lattice([_face(w) for w in axes])
    distinct, face, c = capi.lattice_axes(P)
    assert distinct == 1
    for a in range(3):
        if a in axes:
            assert face[a] == axes.index(a) and c[a] == F32(CONST[a])
        else:
            assert face[a] == -1 and np.isnan(c[a])


def test_two_faces_on_one_axis_keep_the_general_code():
    for faces in ([(2, 0, -0.125), (2, 0, 0.625)], [(2, 0, -0.125), (0, 1, -1.25), (2, 0, 0.625)], [(1, 0, -1.5), (1, 2, 1.5)]):
        P = lattice(faces)
        assert len(capi.lattice_detect(P)) == len(faces)
        distinct, face, c = capi.lattice_axes(P)
        assert distinct == 0 and face == [-1, -1, -1] and np.isnan(c).all()


def test_degenerate_tables():
    # a face of ONE row is no lattice face (cd_lattice_detect wants two entries along both axes): nothing to classify
    one_row = lattice([(2, 0, -0.125)], tabs={0: TABS[0], 1: np.array([0.25]), 2: TABS[2]})
    assert capi.lattice_detect(one_row) == []
    distinct, face, c = capi.lattice_axes(one_row)
    assert distinct == 0 and face == [-1, -1, -1] and np.isnan(c).all()
    # the smallest lattice: one face of 2 x 2 - its constant axis has the single-entry table the kernel gives such an axis
    tiny = lattice([(1, 0, 0.5)], tabs={0: np.array([0.0, 1.0]), 1: TABS[1], 2: np.array([-2.0, 2.0])})
    assert len(capi.lattice_detect(tiny)) == 1
    distinct, face, c = capi.lattice_axes(tiny)
    assert distinct == 1 and face == [-1, 0, -1] and c[1] == F32(0.5)
    # not a lattice at all
    rng = np.random.default_rng(0)
    assert capi.lattice_axes(rng.normal(size=(50, 3)).astype(F32))[0] == 0


def test_reference_templates(template):
    big = pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75.pcd")).astype(F32)
    assert len(capi.lattice_detect(big)) == 6
    assert capi.lattice_axes(big)[0] == 0
    distinct, face, c = capi.lattice_axes(template)        # the launch default: z = -H/2, y = -W/2, x = -L/2
    assert distinct == 1 and face == [2, 1, 0]
    d = templates.DEFAULT_TEMPLATE
    assert c.tolist() == [F32(-d["length"] / 2), F32(-d["width"] / 2), F32(-d["height"] / 2)]
    three = pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75_3faces.pcd")).astype(F32)
    assert capi.lattice_axes(three)[0] == 1
    for dims in synth.CONFIG5_DIMS:                         # config 5's five templates come from the same generator
        assert capi.lattice_axes(templates.template_xyz32(*dims))[0] == 1, dims
