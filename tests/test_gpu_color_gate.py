"""The colour gate on the GPU (k_color_bbox, cd_color_bbox_batch[_device], cd_set_bbox_source / cd_set_frame_bboxes): the device
stage equals canonical rule C10 restated in numpy (perception_amd/color_gate.py) in every field, frames of a batch are
independent, per-frame rectangles gate each frame as the single rectangle of cd_params gates a one-frame call, CD_BBOX_COLOR
equals CD_BBOX_PER_FRAME fed the CPU rectangles, and with the source left alone every call does what it did before."""
import ctypes as C

import numpy as np
import pytest
import torch

from perception_amd import capi, synth
from perception_amd import color_gate as cg
from test_depth_cpu import deproject, synth_camera

pytestmark = pytest.mark.gpu
W, H = synth.WIDTH, synth.HEIGHT
P = W * H
NF = 12      # frames of the fused-chain tests
NBIG = 256   # the batch the stage was built for

RED, RED2, GREY, ORANGE = (200, 30, 40), (200, 90, 40), (150, 140, 130), (200, 150, 40)
FIELDS = ("found", "area2", "n_components", "n_mask")


def _rec(b):
    return {"rect": tuple(b.rect), **{k: int(getattr(b, k)) for k in FIELDS}}


def _check(got, imgs, params=None, what=""):
    for f, img in enumerate(imgs):
        want = cg.color_bbox(img, params)
        assert _rec(got[f]) == want, (what, f, _rec(got[f]), want)


@pytest.fixture(scope="module")
def big():
    c = capi.Context(max_points=P, max_frames=NBIG)
    yield c
    c.close()


@pytest.fixture(scope="module")
def images():
    pairs = [synth.depth_frame(i) for i in range(NF)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.fixture(scope="module")
def ctx(template):
    c = capi.Context(max_points=P, max_frames=NF)
    c.set_template(0, template)
    yield c
    c.close()


def _paint(m, rng=None):
    img = np.empty(m.shape + (3,), np.uint8)
    img[...] = GREY
    img[m] = RED
    if rng is not None:   # both object colours, and background colours outside the mask
        img[m & (rng.random(m.shape) < 0.5)] = RED2
        img[~m & (rng.random(m.shape) < 0.3)] = ORANGE
    return img


def _adversarial(w, h, seed):
    """Seeded images of one size: noise, equal blobs, diagonal joins, a hole, border blobs, all red, all grey."""
    rng = np.random.default_rng(seed)
    out = []
    noise = rng.random((h, w)) < 0.5
    out.append(_paint(noise))
    raw = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)   # every branch of the HSV conversion
    out.append(raw)
    out.append(_paint(rng.random((h, w)) < 0.97, rng))        # mostly red with pin holes: the opening eats around them
    s = max(1, min(w, h) // 4)
    m = np.zeros((h, w), bool)                                # two blobs of equal area2
    m[0:s, 0:s] = True
    m[h - s:h, w - s:w] = True
    out.append(_paint(m, rng))
    m = np.zeros((h, w), bool)                                # blobs joined only diagonally (one component)
    m[0:h // 2, 0:w // 2] = True
    m[h // 2:h, w // 2:w] = True
    out.append(_paint(m))
    m = np.zeros((h, w), bool)                                # anti-diagonal join, away from the border where there is room
    m[h // 2:h - h // 8, w // 8:w // 2] = True
    m[h // 8:h // 2, w // 2:w - w // 8] = True
    out.append(_paint(m, rng))
    m = np.ones((h, w), bool)                                 # a blob with a hole, touching all borders
    m[h // 3:h - h // 3, w // 3:w - w // 3] = False
    out.append(_paint(m))
    m = np.zeros((h, w), bool)                                # blobs on the image border, different sizes
    m[0:max(1, h // 3), w // 4:w // 2] = True
    m[h - max(1, h // 5):h, 0:max(1, w // 3)] = True
    m[h // 3:h // 3 + max(1, h // 4), w - max(1, w // 6):w] = True
    out.append(_paint(m, rng))
    out.append(_paint(np.ones((h, w), bool)))
    out.append(_paint(np.zeros((h, w), bool)))
    if w >= 64 and h >= 64:                                   # many components survive the opening: a grid of 11 x 11 squares
        m = np.zeros((h, w), bool)
        for y in range(2, h - 12, 14):
            for x in range(3, w - 12, 14):
                m[y:y + 11 + (x + y) % 3, x:x + 11] = True
        out.append(_paint(m, rng))
        m = np.zeros((h, w), bool)                            # a comb: long runs, many hooks into one component
        m[4:h - 4, 4:16] = True
        for y in range(4, h - 14, 24):
            m[y:y + 11, 4:w - 4] = True
        out.append(_paint(m))
    return np.stack(out)


def test_synth_batch_256_and_single(big):
    imgs = np.stack([synth.depth_frame(i)[1] for i in range(NBIG)])
    got = big.color_bbox_batch(imgs)
    _check(got, imgs, what="256")
    assert all(got[f].found == 1 for f in range(NBIG))
    t = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    dev = big.color_bbox_batch_device(t)
    assert bytes(dev) == bytes(got)
    one = big.color_bbox_batch(imgs[5:6])
    assert bytes(one)[:32] == bytes(got)[5 * 32:6 * 32]
    # an unaligned device pointer takes the byte-wise load path: same records
    flat = torch.zeros(imgs[:3].size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = t[:3].reshape(-1)
    torch.cuda.synchronize()
    un = big.color_bbox_batch_device(flat[1:].view(3, H, W, 3))
    assert bytes(un)[:96] == bytes(got)[:96]


@pytest.mark.parametrize("w,h", [(640, 480), (320, 240), (33, 17), (8, 8), (1, 1)])
def test_adversarial_images(big, w, h):
    imgs = _adversarial(w, h, 100 + w)
    got = big.color_bbox_batch(imgs)
    _check(got, imgs, what=(w, h))
    t = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    assert bytes(big.color_bbox_batch_device(t)) == bytes(got)
    if w >= 320:
        assert max(got[f].n_components for f in range(len(imgs))) >= 2
        assert any(got[f].found == 0 for f in range(len(imgs)))


def test_images_beyond_the_lds_plan(big):
    """Shapes whose packed mask does not fit LDS run the same code on global memory: very wide, very tall, one pixel wide."""
    for w, h in ((2048, 150), (40, 7000), (1, 20000), (3000, 9)):
        imgs = _adversarial(w, h, 200 + h)[[0, 2, 3, 5, 6, 7]]
        _check(big.color_bbox_batch(imgs), imgs, what=(w, h))


def test_non_default_params(big, images):
    rgb = images[1][:4]
    adv = _adversarial(320, 240, 5)
    for kw in ({"h_lo_max": 20, "margin": 0}, {"h_lo_max": 0, "h_hi_min": 179, "s_min": 200, "v_min": 0, "margin": 3},
               {"h_lo_max": 179, "h_hi_min": 0, "s_min": 0, "v_min": 0, "margin": 25}, {"v_min": 255, "s_min": 255}):
        g = capi.default_color_gate_params()
        for k, v in kw.items():
            setattr(g, k, v)
        for imgs in (rgb, adv):
            _check(big.color_bbox_batch(imgs, g), imgs, g, what=kw)


def test_batch_independence(big, images):
    rgb = images[1]
    blank = np.empty_like(rgb[0])
    blank[...] = GREY
    batch = np.stack([rgb[0], blank, rgb[1], _adversarial(W, H, 9)[3], blank, rgb[2]])
    got = big.color_bbox_batch(batch)
    for f in range(len(batch)):
        alone = big.color_bbox_batch(batch[f:f + 1])
        assert bytes(alone)[:32] == bytes(got)[32 * f:32 * f + 32], f
    assert got[1].found == 0 and tuple(got[1].rect) == (0, 0, 0, 0) and got[4].found == 0
    assert got[0].found == 1 and got[2].found == 1 and got[5].found == 1


def _gate_params(rect=None):
    prm = capi.default_params()
    prm.bbox_enable = 1
    fx, fy, cx, cy = synth.depth_camera_params(W, H)
    Pm = [fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0]
    for i, v in enumerate(Pm):
        prm.bbox_P[i] = v
    if rect is not None:
        for i in range(4):
            prm.bbox_rect[i] = int(rect[i])
    return prm


def _with_offset(prm, off=12):
    prm.rgb_offset = off
    return prm


def _copy(prm):
    q = capi.CdParams()
    C.memmove(C.byref(q), C.byref(prm), C.sizeof(q))
    return q


def _same(a, b, fa, fb):
    """frame fa of call a == frame fb of call b: (results, plane_inliers, labels)"""
    assert bytes(a[0][fa]) == bytes(b[0][fb]), (fa, fb)
    assert np.array_equal(a[1][fa], b[1][fb]) and np.array_equal(a[2][fa], b[2][fb]), (fa, fb)


def test_per_frame_rectangles_equal_single_rectangle_calls(ctx, images):
    depth, rgb = images
    cam = synth_camera()
    clouds = np.stack([deproject(depth[f], rgb[f], cam) for f in range(NF)]).view(np.float32)
    rects = cg.gate_rects(rgb)
    rects[3] = (0, 0, 0, 0)            # keeps nothing
    rects[4] = (-50, -50, 5000, 5000)  # keeps everything
    prm = _with_offset(_gate_params())
    ctx.set_frame_bboxes(rects)
    ctx.set_bbox_source(capi.CD_BBOX_PER_FRAME)
    assert ctx.bbox_source() == capi.CD_BBOX_PER_FRAME
    batch = ctx.process_batch(clouds, prm, want_indices=True)
    used = ctx.frame_bboxes()
    assert [tuple(b.rect) for b in used] == [tuple(r) for r in rects.tolist()]
    t = torch.from_numpy(clouds).cuda()
    torch.cuda.synchronize()
    res_dev = ctx.process_batch_device(t.data_ptr(), 16, P, NF, prm)
    assert bytes(res_dev) == bytes(batch[0])
    one = ctx.process_frame(clouds[2], prm, want_indices=True)   # frame 0 of a one-frame call takes rects[0]
    ctx.set_bbox_source(capi.CD_BBOX_PARAMS)
    ungated = ctx.process_batch(clouds, _with_offset(capi.default_params()), want_indices=True)
    differs = 0
    for f in range(NF):
        single = ctx.process_batch(clouds[f:f + 1], _with_offset(_gate_params(rects[f])), want_indices=True)
        _same(batch, single, f, 0)
        differs += batch[0][f].n_objects != ungated[0][f].n_objects
    assert differs >= 1
    assert batch[0][3].n_objects == 0 and batch[0][4].n_objects == ungated[0][4].n_objects
    single = ctx.process_batch(clouds[2:3], _with_offset(_gate_params(rects[0])), want_indices=True)
    assert bytes(one[0]) == bytes(single[0][0])


def test_color_source_equals_per_frame_fed_the_cpu_rectangles(ctx, images):
    depth, rgb = images
    cam = synth_camera()
    prm = _gate_params()
    rects = cg.gate_rects(rgb)
    want = [cg.color_bbox(rgb[f]) for f in range(NF)]
    assert all(w["found"] == 1 for w in want)
    ctx.set_bbox_source(capi.CD_BBOX_COLOR)
    a = ctx.process_depth_batch(depth, rgb, cam, prm, want_indices=True)
    assert [_rec(b) for b in ctx.frame_bboxes()] == want
    part = ctx.frame_bboxes(first=3, count=2)
    assert len(part) == 2 and tuple(part[0].rect) == want[3]["rect"]
    td, tc = torch.from_numpy(depth.view(np.int16)).cuda().view(torch.uint16), torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    pi, lb = np.empty((NF, P), np.int32), np.empty((NF, P), np.int32)
    res_dev = ctx.process_depth_batch_device(td, tc, cam, prm, plane_inliers=pi, labels=lb)
    assert bytes(res_dev) == bytes(a[0]) and np.array_equal(pi, a[1]) and np.array_equal(lb, a[2])
    assert [_rec(b) for b in ctx.frame_bboxes()] == want
    ctx.set_frame_bboxes(rects)
    ctx.set_bbox_source(capi.CD_BBOX_PER_FRAME)
    b = ctx.process_depth_batch(depth, rgb, cam, prm, want_indices=True)
    for f in range(NF):
        _same(a, b, f, f)
    # the gate does something: against the ungated call
    ungated_prm = capi.default_params()
    c = ctx.process_depth_batch(depth, rgb, cam, ungated_prm, want_indices=True)
    assert any(a[0][f].n_objects != c[0][f].n_objects for f in range(NF))
    assert all(a[0][f].n_objects > 0 for f in range(NF))
    # non-default rule parameters travel with the source
    g = capi.default_color_gate_params()
    g.margin, g.h_lo_max = 0, 4
    ctx.set_bbox_source(capi.CD_BBOX_COLOR, g)
    ctx.process_depth_batch(depth[:3], rgb[:3], cam, prm)
    assert [_rec(b) for b in ctx.frame_bboxes()] == [cg.color_bbox(rgb[f], g) for f in range(3)]
    # with the gate off the source does not matter, and cd_get_frame_bboxes has nothing to report
    ctx.set_bbox_source(capi.CD_BBOX_COLOR)
    d = ctx.process_depth_batch(depth, rgb, cam, ungated_prm, want_indices=True)
    for f in range(NF):
        _same(c, d, f, f)
    with pytest.raises(capi.CuboidError):
        ctx.frame_bboxes()
    ctx.set_bbox_source(capi.CD_BBOX_PARAMS)


def test_default_source_untouched(template, images):
    depth, rgb = images
    cam = synth_camera()
    clouds = np.stack([deproject(depth[f], rgb[f], cam) for f in range(NF)]).view(np.float32)
    c = capi.Context(max_points=P, max_frames=NF)   # a context whose source was never set
    try:
        c.set_template(0, template)
        assert c.bbox_source() == capi.CD_BBOX_PARAMS
        for gated in (False, True):
            prm = _gate_params((200, 150, 420, 330)) if gated else capi.default_params()
            a = c.process_depth_batch(depth, rgb, cam, prm, want_indices=True)
            b = c.process_batch(clouds, _with_offset(_copy(prm)), want_indices=True)
            c.set_frame_bboxes(np.zeros((NF, 4), np.int32))   # stored rectangles alone change nothing
            c.set_bbox_source(capi.CD_BBOX_COLOR)
            c.set_bbox_source(capi.CD_BBOX_PARAMS)
            d = c.process_depth_batch(depth, rgb, cam, prm, want_indices=True)
            for f in range(NF):
                _same(a, b, f, f)
                _same(a, d, f, f)
            if gated:
                assert any(a[0][f].n_objects > 0 for f in range(NF))
    finally:
        c.close()


def test_refusals(ctx, images):
    depth, rgb = images
    cam = synth_camera()
    lib, h = ctx.lib, ctx.h
    prm = _gate_params((0, 0, W, H))
    clouds = np.stack([deproject(depth[f], rgb[f], cam) for f in range(2)]).view(np.float32)
    res = (capi.CdFrameResult * NF)()
    out = (capi.CdColorBBox * NF)()

    def refused(st):
        assert st == capi.CD_ERR_INVALID_ARG, st
        assert lib.cd_last_error(h)

    def raises_invalid(call):
        with pytest.raises(capi.CuboidError) as e:
            call()
        assert e.value.status == capi.CD_ERR_INVALID_ARG and lib.cd_last_error(h)

    def usable():
        _check(ctx.color_bbox_batch(rgb[:2]), rgb[:2])

    ctx.set_bbox_source(capi.CD_BBOX_COLOR)
    raises_invalid(lambda: ctx.process_batch(clouds, _with_offset(_copy(prm))))
    raises_invalid(lambda: ctx.process_frame(clouds[0], _with_offset(_copy(prm))))
    t = torch.from_numpy(clouds).cuda()
    torch.cuda.synchronize()
    refused(lib.cd_process_batch_device(h, C.c_void_p(t.data_ptr()), 16, P, 2, C.byref(_with_offset(_copy(prm))), C.cast(res, C.c_void_p), None, None))
    raises_invalid(lambda: ctx.process_depth_batch(depth[:2], None, synth_camera(color=capi.CD_COLOR_NONE), prm))
    usable()
    ctx.set_bbox_source(capi.CD_BBOX_PER_FRAME)
    ctx.set_frame_bboxes(np.zeros((1, 4), np.int32))
    raises_invalid(lambda: ctx.process_batch(clouds, _with_offset(_copy(prm))))
    raises_invalid(lambda: ctx.process_depth_batch(depth[:2], rgb[:2], cam, prm))
    ctx.set_frame_bboxes(None)
    raises_invalid(lambda: ctx.process_batch(clouds[:1], _with_offset(_copy(prm))))
    ctx.process_batch(clouds[:1], _with_offset(capi.default_params()))   # gate off: no rectangles needed
    usable()
    # the source setter
    refused(lib.cd_set_bbox_source(h, 3, None))
    refused(lib.cd_set_bbox_source(h, -1, None))
    assert ctx.bbox_source() == capi.CD_BBOX_PER_FRAME
    bad = []
    for k, v in (("h_lo_max", -1), ("h_lo_max", 180), ("h_hi_min", -1), ("h_hi_min", 180), ("s_min", -1), ("s_min", 256),
                 ("v_min", -1), ("v_min", 256), ("margin", -1)):
        g = capi.default_color_gate_params()
        setattr(g, k, v)
        bad.append(g)
        refused(lib.cd_set_bbox_source(h, capi.CD_BBOX_COLOR, C.byref(g)))
        assert ctx.bbox_source() == capi.CD_BBOX_PER_FRAME
    ctx.set_bbox_source(capi.CD_BBOX_PARAMS)
    assert lib.cd_get_bbox_source(h, None) == capi.CD_ERR_INVALID_ARG
    # cd_color_bbox_batch[_device]
    a = np.ascontiguousarray(rgb[:2])
    p8 = a.ctypes.data_as(C.c_void_p)
    tc = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    for fn, ptr in ((lib.cd_color_bbox_batch, p8), (lib.cd_color_bbox_batch_device, C.c_void_p(tc.data_ptr()))):
        refused(fn(h, None, W, H, 2, None, out))
        refused(fn(h, ptr, W, H, 2, None, None))
        refused(fn(h, ptr, 0, H, 2, None, out))
        refused(fn(h, ptr, W, 0, 2, None, out))
        refused(fn(h, ptr, -W, -H, 2, None, out))
        refused(fn(h, ptr, W + 1, H, 2, None, out))      # over max_points
        refused(fn(h, ptr, 65536, 65536, 2, None, out))  # the product does not fit int32
        refused(fn(h, ptr, W, H, 0, None, out))
        refused(fn(h, ptr, W, H, -1, None, out))
        refused(fn(h, ptr, W, H, NF + 1, None, out))
        for g in bad:
            refused(fn(h, ptr, W, H, 2, C.byref(g), out))
        assert fn(None, ptr, W, H, 2, None, out) == capi.CD_ERR_INVALID_ARG
    refused(lib.cd_set_frame_bboxes(h, None, 2))
    refused(lib.cd_set_frame_bboxes(h, np.zeros(4, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), -1))
    assert lib.cd_get_frame_bboxes(h, 0, 1, out) == capi.CD_ERR_INVALID_ARG   # no fused call with per-frame rectangles is current
    usable()
    r = ctx.process_depth_batch(depth[:2], rgb[:2], cam, capi.default_params())
    assert r[0][0].status == capi.CD_OK
