"""ctypes wrapper of oracle/liboracle.so - TEST INFRASTRUCTURE ONLY.

May be imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg and by
nothing else; the product package (perception_amd) never imports it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from perception_amd.capi import CdClusterResult, CdFrameResult, CdParams, CdSurfaceFrameResult

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_DIR, "liboracle.so")
_lib = None


def build():
    subprocess.run(["make", "-C", _DIR], check=True, stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_DIR, "cuboid_oracle.cpp")
        if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(src):
            build()
        _lib = C.CDLL(LIB_PATH)
        _lib.orc_pose_to_position_quaternion.restype = None
        _lib.orc_bbox_corners.restype = None
        _lib.orc_bbox_corners.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _pts(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] >= 3
    return a, C.c_size_t(a.strides[0]), a.shape[0]


def mt19937_stream(seed, n):
    out = np.empty(n, np.uint32)
    lib().orc_mt19937_stream(C.c_uint32(seed), n, _p(out))
    return out


def passthrough(points, field, lo, hi):
    a, st, n = _pts(points)
    idx = np.empty(max(n, 1), np.int32)
    cnt = C.c_int()
    lib().orc_passthrough(_p(a), st, n, field, C.c_double(lo), C.c_double(hi), _p(idx), C.byref(cnt))
    return idx[:cnt.value].copy()


def crop_voxel(points, prm, want_rgb=False):
    a, st, n = _pts(points)
    out = np.empty((max(n, 1), 3), np.float32)
    rgb = np.empty(max(n, 1), np.uint32)
    nc, nv = C.c_int(), C.c_int()
    grid = np.zeros(6, np.int32)
    s = lib().orc_crop_voxel(_p(a), st, n, C.byref(prm), _p(out), _p(rgb), n, C.byref(nc), C.byref(nv), _p(grid))
    return s, out[:nv.value].copy(), (rgb[:nv.value].copy() if want_rgb else None), nc.value, grid


def segment_plane(xyz, prm):
    a, st, n = _pts(xyz)
    coeff = np.zeros(4, np.float32)
    inl = np.empty(max(n, 1), np.int32)
    ni, it = C.c_int(), C.c_int()
    s = lib().orc_segment_plane(_p(a), st, n, C.byref(prm), _p(coeff), _p(inl), n, C.byref(ni), C.byref(it))
    return s, coeff, inl[:ni.value].copy(), it.value


def ransac_trace(xyz, prm, cap):
    a, st, n = _pts(xyz)
    tri = np.zeros((cap, 3), np.int32)
    mod = np.zeros((cap, 4), np.float32)
    cnt = np.zeros(cap, np.int32)
    got = C.c_int()
    lib().orc_ransac_trace(_p(a), st, n, C.byref(prm), cap, _p(tri), _p(mod), _p(cnt), C.byref(got))
    g = got.value
    return tri[:g], mod[:g], cnt[:g]


def plane_refit(xyz, inliers, model):
    a, st, n = _pts(xyz)
    inl = np.ascontiguousarray(inliers, np.int32)
    m = np.ascontiguousarray(model, np.float32)
    out = np.zeros(4, np.float32)
    lib().orc_plane_refit(_p(a), st, n, _p(inl), len(inl), _p(m), _p(out))
    return out


def cluster(xyz, prm, mode=1, sizes_capacity=4096):
    a, st, n = _pts(xyz) if len(xyz) else (np.zeros((0, 3), np.float32), C.c_size_t(12), 0)
    labels = np.empty(max(n, 1), np.int32)
    sizes = np.zeros(sizes_capacity, np.int32)
    k = C.c_int()
    lib().orc_cluster(_p(a), st, n, C.byref(prm), mode, _p(labels), _p(sizes), sizes_capacity, C.byref(k))
    return labels[:n].copy(), sizes[:min(k.value, sizes_capacity)].copy(), k.value


def surface_frame(xyz, table_normal, prm, invert=True):
    a, st, n = _pts(xyz)
    tn = np.ascontiguousarray(table_normal, np.float32)
    res = CdSurfaceFrameResult()
    s = lib().orc_surface_frame(_p(a), st, n, _p(tn), 1 if invert else 0, C.byref(prm), C.byref(res))
    return s, res


def bbox_filter(xyz, P, rect):
    a, st, n = _pts(xyz)
    Pm = np.ascontiguousarray(P, np.float64).ravel()
    r = np.ascontiguousarray(rect, np.int32)
    idx = np.empty(max(n, 1), np.int32)
    cnt = C.c_int()
    lib().orc_bbox_filter(_p(a), st, n, _p(Pm), _p(r), _p(idx), C.byref(cnt))
    return idx[:cnt.value].copy()


def nn(tgt, q, mode=0):
    t, ts, m = _pts(tgt)
    a, st, n = _pts(q)
    idx = np.empty(n, np.int32)
    d2 = np.empty(n, np.float32)
    lib().orc_nn(_p(t), ts, m, _p(a), st, n, mode, _p(idx), _p(d2))
    return idx, d2


def icp(tgt, src, prm, nn_mode=1, want_aligned=False):
    t, ts, m = _pts(tgt)
    a, st, n = _pts(src)
    res = CdClusterResult()
    al = np.empty((max(n, 1), 3), np.float32) if want_aligned else None
    s = lib().orc_icp(_p(t), ts, m, _p(a), st, n, C.byref(prm), nn_mode, C.byref(res), _p(al))
    return s, res, (al[:n] if want_aligned else None)


def svd3(A):
    A = np.ascontiguousarray(A, np.float32)
    U = np.zeros((3, 3), np.float32)
    S = np.zeros(3, np.float32)
    V = np.zeros((3, 3), np.float32)
    lib().orc_svd3(_p(A), _p(U), _p(S), _p(V))
    return U, S, V


def umeyama_from_moments(sums, n):
    """umeyama_from_moments on one set of rule C4's 16 sums (uint64) and its count.  Returns (T float32 (4, 4), info dict: rank,
    det_negative (det3(sigma) < 0), uv_positive (det U * det V > 0), S (the float32 singular values))."""
    a = np.ascontiguousarray(sums, np.uint64).reshape(16)
    T = np.zeros(16, np.float32)
    info = np.zeros(6, np.float64)
    lib().orc_umeyama_from_moments(_p(a), int(n), _p(T), _p(info))
    return T.reshape(4, 4), dict(rank=int(info[0]), det_negative=bool(info[1]), uv_positive=bool(info[2]), S=info[3:6].astype(np.float32))


def eigen33_smallest(cov):
    c = np.ascontiguousarray(cov, np.float32)
    v = np.zeros(3, np.float32)
    lib().orc_eigen33_smallest(_p(c), _p(v))
    return v


def mat4_inverse(m):
    a = np.ascontiguousarray(m, np.float64)
    out = np.zeros((4, 4), np.float64)
    s = lib().orc_mat4_inverse(_p(a), _p(out))
    return s, out


def pose_to_position_quaternion(H):
    a = np.ascontiguousarray(H, np.float64)
    pos = np.zeros(3)
    q = np.zeros(4)
    lib().orc_pose_to_position_quaternion(_p(a), _p(pos), _p(q))
    return pos, q


def bbox_corners(H, l, w, h):
    a = np.ascontiguousarray(H, np.float64)
    out = np.zeros((8, 3), np.float32)
    lib().orc_bbox_corners(_p(a), l, w, h, _p(out))
    return out


ARITH_SEQUENTIAL, ARITH_REVERSE_TIES, ARITH_PROBE = 1, 2, 4


def process_frame_arith(arith, points, prm, template, nn_mode=1, all_clusters=32):
    """process_frame under an arithmetic variant (ARITH_* bits of cuboid_oracle.cpp): another execution real PCL's unspecified
    summation / tie orders allow.  Returns dict(result, plane_inliers, labels, clusters)."""
    a, st, n = _pts(points)
    t, ts, m = _pts(template)
    res = CdFrameResult()
    pi = np.empty(max(n, 1), np.int32)
    lb = np.empty(max(n, 1), np.int32)
    allc = (CdClusterResult * max(all_clusters, 1))()
    nall = C.c_int()
    probe = np.zeros(8, np.float64)
    s = lib().orc_process_frame_arith(int(arith), _p(a), st, n, C.byref(prm), _p(t), ts, m, nn_mode, C.byref(res), _p(pi), _p(lb),
                                      allc, all_clusters, C.byref(nall), _p(probe))
    return dict(status=s, result=res, plane_inliers=pi[:max(res.n_plane, 0)].copy(), labels=lb[:max(res.n_objects, 0)].copy(),
                clusters=[allc[i] for i in range(nall.value)], probe=probe)


def process_frame(points, prm, template, nn_mode=1, want_clouds=False, all_clusters=0):
    """One frame through the whole chain.  Returns dict(result, plane_inliers, labels[, voxels, objects][, clusters]).
    all_clusters = capacity of the list of per-cluster ICP results beyond the record's fixed slots (0: record only)."""
    a, st, n = _pts(points)
    t, ts, m = _pts(template)
    res = CdFrameResult()
    pi = np.empty(max(n, 1), np.int32)
    lb = np.empty(max(n, 1), np.int32)
    vox = np.empty((max(n, 1), 3), np.float32) if want_clouds else None
    obj = np.empty((max(n, 1), 3), np.float32) if want_clouds else None
    allc = (CdClusterResult * max(all_clusters, 1))()
    nall = C.c_int()
    s = lib().orc_process_frame_all(_p(a), st, n, C.byref(prm), _p(t), ts, m, nn_mode, C.byref(res), _p(pi), _p(lb),
                                    _p(vox), _p(obj), allc if all_clusters else None, all_clusters, C.byref(nall))
    out = dict(status=s, result=res, plane_inliers=pi[:max(res.n_plane, 0)].copy(),
               labels=lb[:max(res.n_objects, 0)].copy())
    if all_clusters:
        out["clusters"] = [allc[i] for i in range(nall.value)]
    if want_clouds:
        out["voxels"] = vox[:res.n_voxels].copy()
        out["objects"] = obj[:res.n_objects].copy()
    return out
