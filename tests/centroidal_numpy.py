"""The centroidal state block in numpy (tests only): the rows `k_centroidal_state` writes from `(q, v, a)`, computed another
way, and the error bound its float32 tests compare against.

The values come from the spatial algebra of oracle/rbd_numpy.py (Featherstone's [angular; linear] coordinates, dense 6 x 6
transforms, joint by joint from the parent): per body the momentum `I v` and the force `I a + v x* I v` in the body's frame,
without gravity, carried to the world origin by the transposed motion transform and summed, then shifted to the centre of
mass.  The kernel walks every body from the universe in world axes with 3-vectors: the two share the model and nothing else.

The bound.  The kernel's result is a sum over the bodies of products of a mass or an inertia with kinematic vectors, each of
which is itself a sum over the segments of the body's walk (offsets, `w x offset`, joint velocities turned into the world,
`wd x offset`, `w x (w x offset)`, ...).  `terms` below is the sum of the absolute values of all those terms, row by row: the
same walk with every vector replaced by its norm and every difference by a sum.  A computed term carries the rounding of its
factors: a rotation entry after d segments about 8 d eps (a 3 x 3 product: 3 eps; sincos or the quaternion of a value rounded
to the dtype: up to 5 eps), a vector turned by it the same plus its own 3 eps, a double cross product three such factors.
With D the deepest walk of the model that is at most 3 (8 D + 3) + 8 < 32 (D + 2) eps per term, summation included; the
bound is E 32 (D + 2) `terms` with E = eps of the dtype + eps of float64 (the expectation is a float64 result with a rounding
of its own).  It is a bound on the arithmetic, not a measurement: nothing in it is fitted to what the kernel returns.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from jiminy_amd.model import JT_SPHERICAL, CompiledModel
from oracle import rbd_numpy
from oracle.rbd_numpy import _crm, _spatial_inertia, _xform


def _joint(model: CompiledModel, j: int, q: np.ndarray):
    """`rbd_numpy._joint` and the spherical joint it lacks: (R, p) of the joint transform and S in [ang; lin]."""
    if int(model.jtypes[j]) != JT_SPHERICAL:
        return rbd_numpy._joint(model, j, q)
    iq = int(model.idx_q[j])
    x, y, z, w = q[iq:iq + 4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    S = np.zeros((6, 3))
    S[:3] = np.eye(3)
    return R, np.zeros(3), S


def centroidal_of(model: CompiledModel, q: np.ndarray, v: np.ndarray, a: Optional[np.ndarray]) -> np.ndarray:
    """The 15 rows of one state: com, hg (linear, angular), dhg (linear, angular; zeros without `a`)."""
    n = model.njoints
    acc_in = np.zeros(model.nv) if a is None else a
    Xw = [np.eye(6) for _ in range(n)]              # motion transform world -> joint frame
    Rw, pw = [np.eye(3) for _ in range(n)], [np.zeros(3) for _ in range(n)]
    vel, acc = [np.zeros(6) for _ in range(n)], [np.zeros(6) for _ in range(n)]
    h0, f0, mc, mass = np.zeros(6), np.zeros(6), np.zeros(3), 0.0
    for j in range(1, n):
        Rj, pj, S = _joint(model, j, q)
        R, p = model.placement_R[j] @ Rj, model.placement_p[j] + model.placement_R[j] @ pj
        X = _xform(R, p)
        par, iv, nvj = int(model.parents[j]), int(model.idx_v[j]), S.shape[1]
        Xw[j] = X @ Xw[par]
        Rw[j], pw[j] = Rw[par] @ R, pw[par] + Rw[par] @ p
        vj = S @ v[iv:iv + nvj]
        vel[j] = X @ vel[par] + vj
        acc[j] = X @ acc[par] + S @ acc_in[iv:iv + nvj] + _crm(vel[j]) @ vj
        I = _spatial_inertia(model.mass[j], model.com[j], model.inertia[j])
        h = I @ vel[j]
        h0 += Xw[j].T @ h
        f0 += Xw[j].T @ (I @ acc[j] - _crm(vel[j]).T @ h)
        mc += model.mass[j] * (pw[j] + Rw[j] @ model.com[j])
        mass += float(model.mass[j])
    com = mc / mass
    out = np.zeros(15)
    out[0:3], out[3:6], out[6:9] = com, h0[3:], h0[:3] - np.cross(com, h0[3:])
    if a is not None:
        out[9:12], out[12:15] = f0[3:], f0[:3] - np.cross(com, f0[3:])
    return out


def terms_of(model: CompiledModel, q: np.ndarray, v: np.ndarray, a: Optional[np.ndarray]) -> np.ndarray:
    """The sum of the absolute values of the terms of every row (module docstring) of one state."""
    n = model.njoints
    acc_in = np.zeros(model.nv) if a is None else a
    norm = np.linalg.norm
    P, W, V, WD, A = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)    # |p|, |w|, |pd|, |wd|, |pdd| as sums
    t = np.zeros(5)     # com, hg linear, hg angular (about the origin), dhg linear, dhg angular
    mass = 0.0
    for j in range(1, n):
        _, pj, S = _joint(model, j, q)
        par, iv, nvj = int(model.parents[j]), int(model.idx_v[j]), S.shape[1]
        off = norm(model.placement_p[j]) + norm(pj)
        sv, sa = S @ v[iv:iv + nvj], S @ acc_in[iv:iv + nvj]
        wj, lj, awj, alj = norm(sv[:3]), norm(sv[3:]), norm(sa[:3]), norm(sa[3:])
        P[j] = P[par] + off
        W[j] = W[par] + wj
        V[j] = V[par] + W[par] * off + lj
        WD[j] = WD[par] + awj + W[par] * wj
        A[j] = A[par] + WD[par] * off + W[par] ** 2 * off + alj + 2 * W[j] * lj
        m, rc, I = float(model.mass[j]), norm(model.com[j]), norm(model.inertia[j], 2)
        c, vc = P[j] + rc, V[j] + W[j] * rc
        ac = A[j] + WD[j] * rc + W[j] ** 2 * rc
        t += [m * c, m * vc, I * W[j] + c * m * vc, m * ac, I * WD[j] + W[j] * I * W[j] + c * m * ac]
        mass += m
    com = t[0] / mass
    out = np.zeros(15)
    out[0:3], out[3:6], out[6:9] = com, t[1], t[2] + com * t[1]
    if a is not None:
        out[9:12], out[12:15] = t[3], t[4] + com * t[3]
    return out


def depth_of(model: CompiledModel) -> int:
    """Joints on the deepest walk from the universe."""
    depth = np.zeros(model.njoints, dtype=int)
    for j in range(1, model.njoints):
        depth[j] = depth[int(model.parents[j])] + 1
    return int(depth.max())


def run(model: CompiledModel, q: np.ndarray, v: np.ndarray, a: Optional[np.ndarray], dtype=np.float64) -> Dict[str, np.ndarray]:
    """Every lane of `[rows][B]` arrays: `centroidal` `[15][B]` in float64 and `bound`, the error bound of a kernel of `dtype`."""
    B = q.shape[1]
    lanes = lambda f: np.stack([f(model, q[:, b], v[:, b], None if a is None else a[:, b]) for b in range(B)], axis=1)      # noqa: E731
    E = float(np.finfo(np.dtype(dtype)).eps) + float(np.finfo(np.float64).eps)
    return {"centroidal": lanes(centroidal_of), "bound": E * 32 * (depth_of(model) + 2) * lanes(terms_of)}
