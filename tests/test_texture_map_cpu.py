"""Unregistered depth + colour pairs without a GPU: the cd_color_camera mirror of the binding, canonical rule C12
restated in numpy (perception_amd/texture_map.py) - the contract the device mapping (tests/test_gpu_texture_map.py) is held to
byte for byte - against the host entry cd_texture_project bit for bit, against rule C7 in the registered special case, and
against the geometry of synth's two-camera render."""
import ctypes as C

import numpy as np
import pytest

from conftest import rot_xyz
from perception_amd import capi, synth
from perception_amd import texture_map as tm
from test_depth_cpu import QNAN, deproject, synth_camera

BASELINE_X = 0.015      # metres between the two cameras of the geometry test (the D435's is of this order)


def _project_c(cam, cc, u, v, d):
    """cd_texture_project on arrays of pixels: (xyz uint32 (n, 3), iu, iv, textured)."""
    lib = capi.load_library()
    n = len(u)
    xyz = np.zeros((n, 3), np.float32)
    pix = np.zeros((n, 2), np.int32)
    tex = np.zeros(n, np.int32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    px, pp, pt = xyz.ctypes.data, pix.ctypes.data, tex.ctypes.data
    for i in range(n):
        st = lib.cd_texture_project(C.byref(cam), C.byref(cc), int(u[i]), int(v[i]), int(d[i]), C.cast(px + 12 * i, f32p),
                                    C.cast(pp + 8 * i, i32p), C.cast(pt + 4 * i, i32p))
        assert st == capi.CD_OK, i
    return xyz.view(np.uint32), pix[:, 0], pix[:, 1], tex.astype(bool)


def _project_np(cam, cc, u, v, d):
    """The restatement on the same pixels: each one is pixel (u, v) of an image of its own row."""
    out = []
    for i in range(len(u)):
        w = int(u[i]) + 1
        img = np.zeros((int(v[i]) + 1, w), np.uint16)
        img[v[i], u[i]] = d[i]
        xyz, iu, iv, tex = tm.project(img, cam, cc)
        k = int(v[i]) * w + int(u[i])
        out.append((xyz[k].view(np.uint32), iu[k], iv[k], tex[k]))
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out], bool))


def _same(a, b, what=""):
    for x, y, name in zip(a, b, ("xyz", "iu", "iv", "textured")):
        assert np.array_equal(x, y), (what, name, np.argwhere(np.asarray(x) != np.asarray(y))[:4])


def test_color_camera_struct_matches_header():
    lib = capi.load_library()
    assert lib.cd_color_camera_struct_size() == C.sizeof(capi.CdColorCamera) == 80
    assert lib.cd_struct_size(9) == -1 and lib.cd_abi_version() == 4       # the closed list and the ABI version stay
    a = capi.CdColorCamera()
    lib.cd_default_color_camera(C.byref(a))
    b = capi.default_color_camera()
    for name, _ in capi.CdColorCamera._fields_:
        x, y = getattr(a, name), getattr(b, name)
        if hasattr(x, "__len__"):
            x, y = list(x), list(y)
        assert x == y, name
    assert (a.width, a.height, a.no_texture) == (640, 480, capi.CD_NOTEX_DROP)
    assert list(a.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(a.t) == [0, 0, 0]
    assert a.fx == np.float32(616.8246459960938) and a.fy == np.float32(616.609375)


@pytest.mark.parametrize("mode", [capi.CD_NOTEX_DROP, capi.CD_NOTEX_KEEP])
def test_texture_project_equals_the_restatement_on_a_seeded_sweep(mode):
    """12 000 pixels in 60 camera pairs: depths (zeros among them), both intrinsics, small rotations and translations - whole
    images through the restatement, pixel by pixel through cd_texture_project."""
    rng = np.random.default_rng(20190409 + mode)
    lib = capi.load_library()
    n_tex = n_out = n_zero = 0
    for pair in range(60):
        w, h = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        cam = synth_camera(w, h)
        cam.fx, cam.fy = rng.uniform(5, 60, 2)
        cam.cx, cam.cy = rng.uniform(-2, w + 2), rng.uniform(-2, h + 2)
        cam.depth_scale = float(rng.choice([0.001, 0.000125, 0.01]))
        cw, ch = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        Rm = rot_xyz(*rng.uniform(-0.08, 0.08, 3))
        cc = capi.color_camera(cw, ch, K=(rng.uniform(5, 90), rng.uniform(5, 90), rng.uniform(0, cw), rng.uniform(0, ch)), R=Rm,
                               t=rng.uniform(-0.05, 0.05, 3), no_texture=mode)
        idx = rng.integers(0, w * h, 200)
        v, u = np.divmod(idx, w)
        img = rng.integers(1, 3000, (h, w)).astype(np.uint16)
        img[rng.random((h, w)) < 0.1] = 0
        xyz, iu, iv, tex = tm.project(img, cam, cc)
        got = _project_c(cam, cc, u, v, img[v, u])
        _same(got, (xyz[idx].view(np.uint32), iu[idx], iv[idx], tex[idx]), pair)
        n_tex += int(tex[idx].sum())
        n_zero += int((img[v, u] == 0).sum())
        n_out += int((~tex[idx] & (img[v, u] != 0)).sum())
        assert ((iu[idx] == -1) == ~tex[idx]).all() and ((iv[idx] == -1) == ~tex[idx]).all()
        assert lib.cd_texture_project(C.byref(cam), C.byref(cc), 0, 0, 1, None, None, None) == capi.CD_OK   # outputs are optional
    assert n_tex > 2000 and n_out > 2000 and n_zero > 500, (n_tex, n_out, n_zero)


def test_hand_made_pixels():
    f32 = np.float32
    cam = synth_camera(8, 4)
    cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale = 2.0, 2.0, 0.0, 0.0, 0.001
    # colour camera: fx 2 as well, so pu = u + ccx exactly while R = I, t = 0
    for mode in (capi.CD_NOTEX_DROP, capi.CD_NOTEX_KEEP):
        keep = mode == capi.CD_NOTEX_KEEP
        cc = capi.color_camera(4, 3, K=(2.0, 2.0, 0.5, 0.0), no_texture=mode)
        u = np.array([0, 0, 1, 3, 4, 0])
        v = np.array([0, 1, 2, 0, 0, 3])
        d = np.array([0, 1000, 1000, 1000, 1000, 1000])
        got = _project_c(cam, cc, u, v, d)
        _same(got, _project_np(cam, cc, u, v, d), "half pixel")
        xyz, iu, iv, tex = got
        assert (xyz[0] == QNAN).all() and not tex[0] and (iu[0], iv[0]) == (-1, -1)          # d == 0, in both modes
        # pu = u + 0.5 exactly: the half-pixel boundary goes UP (floor(pu + 0.5) = u + 1)
        assert tex[1] and (iu[1], iv[1]) == (1, 1) and tex[2] and (iu[2], iv[2]) == (2, 2)
        assert xyz[1].view(f32).tolist() == [0.0, 0.5, 1.0]
        # u = 3 -> iu = 4 = cw: outside by one; v = 3 -> iv = 3 = ch: outside by one
        for k in (3, 5):
            assert not tex[k] and (iu[k], iv[k]) == (-1, -1), k
            assert (xyz[k] == QNAN).all() != keep, k
        assert xyz[4].view(f32)[2] == f32(1.0) if keep else (xyz[4] == QNAN).all()
        # iu = -1: ccx = -1.5 puts pixel u = 0 at pu = -1.5 -> floor(-1.0) = -1; at ccx = -0.5 it is pu = -0.5 -> floor(0.0) = 0
        cc_l = capi.color_camera(4, 3, K=(2.0, 2.0, -1.5, 0.0), no_texture=mode)
        cc_0 = capi.color_camera(4, 3, K=(2.0, 2.0, -0.5, 0.0), no_texture=mode)
        one = (np.array([0]), np.array([0]), np.array([1000]))
        a, b = _project_c(cam, cc_l, *one), _project_c(cam, cc_0, *one)
        _same(a, _project_np(cam, cc_l, *one), "iu = -1")
        _same(b, _project_np(cam, cc_0, *one), "iu = 0")
        assert not a[3][0] and a[1][0] == -1 and b[3][0] and (b[1][0], b[2][0]) == (0, 0)
        # Zc <= 0: behind the colour camera (t_z = -2 m), and exactly in its plane (t_z = -1 m at z = 1 m: Xc / 0)
        for tz in (-2.0, -1.0):
            cc_b = capi.color_camera(4, 3, K=(2.0, 2.0, 0.5, 0.0), t=(0.0, 0.0, tz), no_texture=mode)
            pts = (np.array([0, 1]), np.array([0, 1]), np.array([1000, 1000]))
            g = _project_c(cam, cc_b, *pts)
            _same(g, _project_np(cam, cc_b, *pts), ("Zc", tz))
            assert not g[3].any() and (g[1] == -1).all()
            assert ((g[0] == QNAN).all(axis=1) != keep).all()
        # a non-finite projection with Zc > 0: the quotient overflows float32
        cc_i = capi.color_camera(4, 3, K=(3.0e38, 2.0, 0.5, 0.0), no_texture=mode)
        pts = (np.array([7]), np.array([0]), np.array([1000]))
        g = _project_c(cam, cc_i, *pts)
        _same(g, _project_np(cam, cc_i, *pts), "overflow")
        with np.errstate(over="ignore"):
            assert np.isinf(f32(3.5) * f32(3.0e38))
        assert not g[3][0] and g[1][0] == -1


def test_refused_cameras():
    lib = capi.load_library()
    cam, cc = synth_camera(), capi.default_color_camera()
    call = lambda a, b, u=0, v=0: lib.cd_texture_project(None if a is None else C.byref(a), None if b is None else C.byref(b), u, v, 1, None, None, None)
    assert call(cam, cc) == capi.CD_OK
    assert call(None, cc) == capi.CD_ERR_INVALID_ARG and call(cam, None) == capi.CD_ERR_INVALID_ARG
    assert call(cam, cc, u=-1) == capi.CD_ERR_INVALID_ARG and call(cam, cc, v=-1) == capi.CD_ERR_INVALID_ARG
    bad = [capi.color_camera(width=0), capi.color_camera(height=-1), capi.color_camera(no_texture=2), capi.color_camera(no_texture=-1)]
    for k in (0, 1):
        for val in (0.0, -1.0, np.nan, np.inf):
            K = [600.0, 600.0, 320.0, 240.0]
            K[k] = val
            bad.append(capi.color_camera(K=K))
    for i in range(9):
        for val in (np.nan, np.inf, -np.inf):
            Rm = np.eye(3).ravel()
            Rm[i] = val
            bad.append(capi.color_camera(R=Rm))
    for i in range(3):
        tv = np.zeros(3)
        tv[i] = np.nan
        bad.append(capi.color_camera(t=tv))
    for b in bad:
        assert call(cam, b) == capi.CD_ERR_INVALID_ARG
    for name in ("fx", "fy", "depth_scale"):
        c2 = synth_camera()
        setattr(c2, name, 0.0)
        assert call(c2, cc) == capi.CD_ERR_INVALID_ARG, name


def test_registered_special_case_is_rule_c7():
    """ccam = the depth camera's size and K, R = I, t = 0: every valid pixel maps to itself and its four words are rule C7's;
    a pixel with d == 0 differs only in the rgb word (C7 gives it its own colour, C12 has no point to project)."""
    cam = synth_camera()
    cc = capi.color_camera(cam.width, cam.height, K=(cam.fx, cam.fy, cam.cx, cam.cy))
    v, u = np.divmod(np.arange(cam.width * cam.height), cam.width)
    for i in range(2):
        depth, rgb = synth.depth_frame(i)
        for mode in (capi.CD_NOTEX_DROP, capi.CD_NOTEX_KEEP):
            cc.no_texture = mode
            rec, iu, iv, tex = tm.texture_map(depth, rgb, cam, cc)
            ref = deproject(depth, rgb, cam)
            ok = depth.reshape(-1) != 0
            assert np.array_equal(tex, ok)
            assert np.array_equal(iu[ok], u[ok]) and np.array_equal(iv[ok], v[ok])
            assert np.array_equal(rec[ok], ref[ok])
            assert np.array_equal(rec[~ok, :3], ref[~ok, :3]) and (rec[~ok, :3] == QNAN).all() and not rec[~ok, 3].any()
            assert ref[~ok, 3].any() and 0 < (~ok).sum() < ok.sum()


def _uniform3x3(img):
    """(h, w) bool: the 3 x 3 neighbourhood of the pixel (clipped at the border) has one colour."""
    p = (img[..., 0].astype(np.int64) << 16) | (img[..., 1].astype(np.int64) << 8) | img[..., 2]
    h, w = p.shape
    pad = np.pad(p, 1, mode="edge")
    out = np.ones((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out &= pad[dy:dy + h, dx:dx + w] == p
    return out


def test_geometry_on_the_two_camera_render():
    """A colour camera at the README's colour K, 15 mm to the side: a textured point's colour is the colour render() gave its
    depth pixel wherever the colour image is uniform around (iu, iv) and the colour camera sees the point (its own depth
    rendering agrees with Zc within 2 mm).  The checked set must hold at least 80 % of the textured points.
    The restatement alone, frames 0 / 1 / 2: 82.3 % / 82.0 % / 80.5 % checked (the depth noise of 1.2 - 2 mm at these ranges is
    what the 2 mm test drops; the 3 x 3 test drops under 1 %), no mismatch inside the checked set, 107 / 245 / 236 outside it."""
    cam = synth_camera()
    cc = capi.color_camera(t=(BASELINE_X, 0.0, 0.0))
    Rm, tv = np.array(list(cc.R)).reshape(3, 3), np.array(list(cc.t))
    for i in range(3):
        depth, rgb = synth.unregistered_frame(i, cc)
        assert rgb.shape == (cc.height, cc.width, 3) and rgb.dtype == np.uint8
        assert np.array_equal(depth, synth.depth_frame(i)[0])
        crgb, zc = synth.render_color_camera(synth.scene_for(i), cc)
        assert np.array_equal(crgb, rgb)
        rec, iu, iv, tex = tm.texture_map(depth, rgb, cam, cc)
        m = np.flatnonzero(tex)
        assert 0.3 < len(m) / tex.size < 0.45
        pz = (rec[m, :3].view(np.float32).astype(np.float64) @ Rm.T + tv)[:, 2]
        sees = np.abs(zc[iv[m], iu[m]] - pz) <= 0.002
        checked = sees & _uniform3x3(rgb)[iv[m], iu[m]]
        share = checked.mean()
        print("frame %d: %.1f %% of %d textured points checked" % (i, 100 * share, len(m)))
        assert share >= 0.8, (i, share)
        want = synth.depth_frame(i)[1].reshape(-1, 3)[m].astype(np.uint32)
        want = (want[:, 0] << 16) | (want[:, 1] << 8) | want[:, 2]
        assert np.array_equal(rec[m, 3][checked], want[checked]), i
        # both box and table colours are among the checked points
        assert len(np.unique(want[checked])) >= 2


def test_share_of_depth_pixels_inside_the_colour_image():
    """README pair, identity extrinsics, constant depth: the colour camera's narrower field of view holds 38.8 % of the depth
    image's pixels - a guard on the in-range test of step 5."""
    cam, cc = capi.default_depth_camera(), capi.default_color_camera()
    d = np.full((480, 640), 1000, np.uint16)
    rec, iu, iv, tex = tm.texture_map(d, np.zeros((480, 640, 3), np.uint8), cam, cc)
    assert abs(tex.mean() - 0.388) < 0.0005, tex.mean()
    inside = tex.reshape(480, 640)
    rows, cols = np.flatnonzero(inside.any(axis=1)), np.flatnonzero(inside.any(axis=0))
    assert inside[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all()          # one rectangle
    # (the colour camera magnifies 1.6 x: the depth pixels reach its borders but skip colour pixels in between)
    assert iu[tex].min() <= 1 and iu[tex].max() >= 638 and iv[tex].min() <= 1 and iv[tex].max() >= 478
    assert (rec[~tex, :3] == QNAN).all() and not rec[:, 3].any()
