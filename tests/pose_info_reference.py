"""References for the pose-information tests (rule C23), CPU only.

  * expected(): the result of a fused call with the rule on, composed from the records of tests/fused_reference.py - the oracle's
    front end, clustering and ICP - and, for every cluster, perception_amd/pose_info.py on (the cluster's points as extracted, the
    kept pair's T, the kept slot's template, the kept pair's `accepted`).  The rule changes no record of the call, so everything
    the composed reference returns stays and every frame gains "pose_info" (with rule C21 on as well: "scores");
  * information_f64(): the information matrix written from its definition, J^T J in float64, with none of the rule's sums;
  * published_pose() / numeric_ros_jacobian(): the pose a node publishes, P = T^-1, under the rule's perturbation model, and its
    derivative by central differences."""
import numpy as np

import fused_reference as FR
import pair_score_reference as PSR
from perception_amd import icp_plane as IP, pair_score as PS, pose_info as PI

EMPTY = np.zeros((0, 3), np.float32)


def info_of(cluster, templates_by_slot, setting):
    """setting: (max_range, min_support)."""
    return PI.pose_info(cluster.points, cluster.T, templates_by_slot.get(cluster.slot, EMPTY), setting[0], setting[1], cluster.accepted)


def expected(frames, prm, templates_by_slot, opt, setting, pair_setting=None):
    out = FR.expected(frames, prm, templates_by_slot, opt)
    for e in out:
        e["pose_info"] = [info_of(c, templates_by_slot, setting) for c in e["clusters"]]
        if pair_setting is not None:
            e["scores"] = [PSR.score_of(c, templates_by_slot, pair_setting) for c in e["clusters"]]
    return out


def information_f64(src, T, tpl, max_range):
    """H = J^T J over x = (L omega, t), float64: the row of a kept point is ((p x e_w) / L, e_w), p = A - c0 - with A, the neighbour,
    the face and the bound taken from the rule (float32), everything after that in float64."""
    tpl = np.asarray(tpl, np.float32).reshape(-1, 3)
    A = PS.aligned(T, src)
    idx, d2 = IP.nearest(tpl, A)
    keep = d2 <= PS.tau_of(max_range)
    w = IP.face_axes(tpl)[idx[keep]]
    c0, L = PI.box_of(tpl)
    p = A[keep].astype(np.float64) - c0.astype(np.float64)[None, :]
    e = np.eye(3)[w]
    J = np.concatenate([np.cross(p, e) / L, e], axis=1)
    return J.T @ J


def _rot(omega):
    """exp([omega]x), Rodrigues."""
    th = np.linalg.norm(omega)
    K = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if th < 1e-300:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)


def published_pose(T, c0, omega, t):
    """P' = (delta T)^-1 for the motion delta: A -> c0 + R(omega) (A - c0) + t of the template frame (to first order the rule's
    A' = A + omega x (A - c0) + t): (position, rotation matrix)."""
    D = np.eye(4)
    D[:3, :3] = _rot(np.asarray(omega, np.float64))
    D[:3, 3] = np.asarray(c0, np.float64) - D[:3, :3] @ np.asarray(c0, np.float64) + np.asarray(t, np.float64)
    P = np.linalg.inv(D @ np.asarray(T, np.float64).reshape(4, 4))
    return P[:3, 3].copy(), P[:3, :3].copy()


def numeric_ros_jacobian(T, c0, h=1e-6):
    """d(position, rotation about the fixed axes of the parent frame) / d(omega, t) by central differences: 6 x 6.  The rotation
    between two poses P-, P+ about fixed axes is the vector of R+ R-^T."""
    J = np.zeros((6, 6))
    for k in range(6):
        x = np.zeros(6)
        x[k] = h
        pp, Rp = published_pose(T, c0, x[:3], x[3:])
        pm, Rm = published_pose(T, c0, -x[:3], -x[3:])
        dR = Rp @ Rm.T
        J[:3, k] = (pp - pm) / (2 * h)
        J[3:, k] = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0 / (2 * h)
    return J
