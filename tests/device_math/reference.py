"""Plain restatements of the math of jiminy_amd/csrc/jm_math.h, for tests/test_device_math.py and
tools/make_device_math_fixtures.py.

Every composite is written once against a small number-system interface `F` and evaluated three ways:

* `REF` (Python floats + libm): the reference's formula in float64 -- Pinocchio v2.7 (exp6, log3, quaternion::exp3 /
  log3, Jlog3) and Eigen (quaternion from a rotation matrix) with their own branches and Taylor thresholds, true
  divisions instead of the kernels' `rcp_`;
* `REF32` (NumPy float32 scalars): the same formula in float32, with the float32 thresholds;
* `MP` (mpmath): the truth.  It takes the reference's branch where the branches are different exact formulas (log3 near
  pi, the four cases of the quaternion) and the exact expression where the reference truncates a Taylor series.
"""
from __future__ import annotations

import math

import numpy as np

TAYLOR = {np.float64: 2.0 ** -13, np.float32: float(np.float32(1.1920929e-7) ** np.float32(0.25))}  # eps^(1/4)
LOG3_PI_MARGIN = 1e-2
# output groups of every composite (rows of the probe's output): errors are measured in ulps of the largest |truth| of a group
GROUPS = {"exp6": ((0, 9), (9, 12)), "log3": ((0, 3),), "matrix_to_quat": ((0, 4),), "quat_to_matrix": ((0, 9),),
          "quat_exp3": ((0, 4),), "quat_log3": ((0, 3), (3, 4)), "quat_mul": ((0, 4),), "jlog3_mul": ((0, 3),),
          "sym_inverse": ((0, 6),), "rot_rodrigues": ((0, 9),)}


class _Ref:
    exact = False
    sin, cos, sqrt, acos, atan2 = math.sin, math.cos, math.sqrt, math.acos, math.atan2
    pi = math.pi

    @staticmethod
    def num(x):
        return float(x)


class _Ref32:
    """the reference's formula in float32 (NumPy scalars: every operation rounds to float32, Python constants included)"""
    exact = False
    pi = math.pi

    @staticmethod
    def num(x):
        return np.float32(x)

    @staticmethod
    def sin(x):
        return np.sin(np.float32(x))

    @staticmethod
    def cos(x):
        return np.cos(np.float32(x))

    @staticmethod
    def sqrt(x):
        return np.sqrt(np.float32(x))

    @staticmethod
    def acos(x):
        return np.arccos(np.float32(x))

    @staticmethod
    def atan2(y, x):
        return np.arctan2(np.float32(y), np.float32(x))


class _Mp:
    exact = True

    def __init__(self):
        import mpmath
        self.m = mpmath.mp
        self.sin, self.cos, self.sqrt, self.acos, self.atan2 = mpmath.sin, mpmath.cos, mpmath.sqrt, mpmath.acos, mpmath.atan2

    @property
    def pi(self):
        return self.m.pi

    def num(self, x):
        return self.m.mpf(float(x))


REF = _Ref()
REF32 = _Ref32()


def ref32(op: str, x: np.ndarray):
    """(outputs, branch) of the reference's formula evaluated in float32, row by row"""
    out, br = [], []
    with np.errstate(all="ignore"):
        for row in x:
            o, b = COMPOSITES[op](REF32, [np.float32(v) for v in row], np.float32)
            out.append([float(v) for v in o])
            br.append(b)
    return np.array(out), br


def mp_system(dps: int = 60) -> _Mp:
    import mpmath
    mpmath.mp.dps = dps
    return _Mp()


# ---- composites: f(F, a, dtype, branch) -> (outputs, branch taken); `a` the probe's input row
def exp6(F, a, dtype, br=None):
    v, w = [F.num(x) for x in a[:3]], [F.num(x) for x in a[3:6]]
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    t = F.sqrt(t2)
    small = t < TAYLOR[dtype] if br is None else br
    if F.exact:
        if t2 == 0:
            awxv, av, aw, dg = F.num(0.5), F.num(1), 1 / F.num(6), F.num(1)
        else:
            st, ct = F.sin(t), F.cos(t)
            awxv, av, dg = (1 - ct) / t2, st / t, ct
            aw = (t - st) / (t2 * t)
    elif small:
        awxv, av, aw, dg = 0.5 - t2 / 24.0, 1.0 - t2 / 6.0, 1.0 / 6.0 - t2 / 120.0, 1.0 - t2 / 2.0
    else:
        st, ct = F.sin(t), F.cos(t)
        inv_t2 = 1.0 / t2
        awxv, av = (1.0 - ct) * inv_t2, st / t
        aw, dg = (1.0 - av) * inv_t2, ct
    wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2]
    c = (w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0])
    p = [av * v[i] + (aw * wv) * w[i] + awxv * c[i] for i in range(3)]
    R = [awxv * w[0] * w[0] + dg, awxv * w[0] * w[1] - av * w[2], awxv * w[0] * w[2] + av * w[1],
         awxv * w[1] * w[0] + av * w[2], awxv * w[1] * w[1] + dg, awxv * w[1] * w[2] - av * w[0],
         awxv * w[2] * w[0] - av * w[1], awxv * w[2] * w[1] + av * w[0], awxv * w[2] * w[2] + dg]
    return R + p, small


def log3(F, a, dtype, br=None):
    R = [F.num(x) for x in a]
    tr = R[0] + R[4] + R[8]
    if tr >= 3:
        tr, theta = F.num(3), F.num(0)
    elif tr <= -1:
        tr, theta = F.num(-1), F.pi if F.exact else F.num(math.pi)
    else:
        theta = F.acos((tr - 1) / 2)
    near_pi = (theta >= F.num(math.pi) - F.num(LOG3_PI_MARGIN)) if br is None else br
    if near_pi:
        cphi = -(tr - 1) / 2
        beta = theta * theta / (1 + cphi)
        t = [(R[0] + cphi) * beta, (R[4] + cphi) * beta, (R[8] + cphi) * beta]
        sg = [1 if R[7] > R[5] else -1, 1 if R[2] > R[6] else -1, 1 if R[3] > R[1] else -1]
        return [sg[i] * (F.sqrt(t[i]) if t[i] > 0 else 0 * t[i]) for i in range(3)], near_pi
    if F.exact:
        k = (theta / F.sin(theta) if theta != 0 else F.num(1)) / 2
    else:
        k = (theta / F.sin(theta) if theta > TAYLOR[dtype] else 1.0) / 2.0
    return [k * (R[7] - R[5]), k * (R[2] - R[6]), k * (R[3] - R[1])], near_pi


def matrix_to_quat(F, a, dtype, br=None):
    m = [F.num(x) for x in a]
    M = lambda i, j: m[3 * i + j]
    t = m[0] + m[4] + m[8]
    if br is None:
        if t > 0:
            br = -1
        else:
            br = 0
            if M(1, 1) > M(0, 0):
                br = 1
            if M(2, 2) > M(br, br):
                br = 2
    q = [None] * 4
    if br == -1:
        t = F.sqrt(t + 1)
        q[3] = t / 2
        t = F.num(0.5) / t
        q[0], q[1], q[2] = (M(2, 1) - M(1, 2)) * t, (M(0, 2) - M(2, 0)) * t, (M(1, 0) - M(0, 1)) * t
    else:
        i = br
        j, k = (i + 1) % 3, (i + 2) % 3
        t = F.sqrt(M(i, i) - M(j, j) - M(k, k) + 1)
        q[i] = t / 2
        t = F.num(0.5) / t
        q[3] = (M(k, j) - M(j, k)) * t
        q[j] = (M(j, i) + M(i, j)) * t
        q[k] = (M(k, i) + M(i, k)) * t
    return q, br


def quat_to_matrix(F, a, dtype, br=None):
    x, y, z, w = [F.num(v) for v in a]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
            1 - (txx + tyy)], None


def quat_exp3(F, a, dtype, br=None):
    v = [F.num(x) for x in a]
    t2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    big = (t2 > TAYLOR[dtype]) if br is None else br
    if F.exact:
        th = F.sqrt(t2)
        k, w = (F.sin(th / 2) / th, F.cos(th / 2)) if t2 != 0 else (F.num(0.5), F.num(1))
    elif big:
        th = F.sqrt(t2)
        k, w = F.sin(0.5 * th) / th, F.cos(0.5 * th)
    else:
        k, w = 0.5 - t2 / 48.0, 1.0 - t2 * 0.125
    return [k * v[0], k * v[1], k * v[2], w], big


def quat_log3(F, a, dtype, br=None):
    x, y, z, w = [F.num(v) for v in a]
    n2 = x * x + y * y + z * z
    n = F.sqrt(n2)
    sgn = 1 if w >= 0 else -1
    theta = 2 * F.atan2(n, sgn * w)
    big = (n2 > TAYLOR[dtype]) if br is None else br
    if F.exact:
        k = sgn * theta / n if n2 != 0 else sgn * 2 / abs(w)
    elif big:
        k = sgn * theta / n
    else:
        k = sgn * (2.0 / abs(w)) * (1.0 - n2 / (3.0 * w * w))
    return [k * x, k * y, k * z, theta], big


def quat_mul(F, a, dtype, br=None):
    A, B = [F.num(v) for v in a[:4]], [F.num(v) for v in a[4:]]
    return [A[3] * B[0] + A[0] * B[3] + A[1] * B[2] - A[2] * B[1], A[3] * B[1] + A[1] * B[3] + A[2] * B[0] - A[0] * B[2],
            A[3] * B[2] + A[2] * B[3] + A[0] * B[1] - A[1] * B[0], A[3] * B[3] - A[0] * B[0] - A[1] * B[1] - A[2] * B[2]], None


def jlog3_mul(F, a, dtype, br=None):
    theta, lg, v = F.num(a[0]), [F.num(x) for x in a[1:4]], [F.num(x) for x in a[4:7]]
    small = (theta < TAYLOR[dtype]) if br is None else br
    if F.exact and theta == 0:
        alpha, diag = 1 / F.num(12), F.num(1)
    elif small and not F.exact:
        alpha, diag = 1.0 / 12.0 + theta * theta / 720.0, 0.5 * (2.0 - theta * theta / 6.0)
    else:
        st, ct = F.sin(theta), F.cos(theta)
        if 1 - ct == 0:
            return [math.copysign(math.inf, -st * x) if x != 0 else math.nan for x in lg], small
        s1 = st / (1 - ct)
        alpha, diag = 1 / (theta * theta) - s1 / (2 * theta), (theta * s1) / 2
    d = alpha * (lg[0] * v[0] + lg[1] * v[1] + lg[2] * v[2])
    c = (lg[1] * v[2] - lg[2] * v[1], lg[2] * v[0] - lg[0] * v[2], lg[0] * v[1] - lg[1] * v[0])
    return [d * lg[i] + diag * v[i] + c[i] / 2 for i in range(3)], small


def sym_inverse(F, a, dtype, br=None):
    xx, xy, xz, yy, yz, zz = [F.num(v) for v in a]
    c00, c01, c02 = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
    idet = 1 / (xx * c00 + xy * c01 + xz * c02)
    return [c00 * idet, c01 * idet, c02 * idet, (xx * zz - xz * xz) * idet, (xy * xz - xx * yz) * idet,
            (xx * yy - xy * xy) * idet], None


def rot_rodrigues(F, a, dtype, br=None):
    x, y, z, c, s = [F.num(v) for v in a]
    oc = 1 - c
    return [c + oc * x * x, oc * x * y - s * z, oc * x * z + s * y, oc * y * x + s * z, c + oc * y * y, oc * y * z - s * x,
            oc * z * x - s * y, oc * z * y + s * x, c + oc * z * z], None


COMPOSITES = {f.__name__: f for f in (exp6, log3, matrix_to_quat, quat_to_matrix, quat_exp3, quat_log3, quat_mul, jlog3_mul,
                                      sym_inverse, rot_rodrigues)}


# ---- ulps
def ulp(x, dtype=np.float64) -> np.ndarray:
    """Spacing of `dtype` at |x| (the smallest denormal at 0)."""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(dtype)
    return np.spacing(a).astype(np.float64)


def ulp_err(got, hi, lo, dtype=np.float64) -> np.ndarray:
    """|got - (hi + lo)| in ulps of `dtype` at the truth (exact in double-double: got - hi is exact for nearby values)."""
    got = np.asarray(got, dtype=np.float64)
    return np.abs((got - hi) - lo) / ulp(hi, dtype)


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


# pi/2 in pieces of 32 significant bits (k * piece is exact for k < 2^21); the rest is below 2^-176
_PIO2 = tuple(float.fromhex(h) for h in ("0x1.921fb544p+0", "0x1.0b4611a6p-34", "0x1.3198a2e0p-69", "0x1.b839a252p-104",
                                         "0x1.27044534p-142"))


def kgrid_truth(k: np.ndarray, x: np.ndarray):
    """sin and cos of x = k pi/2 + d, |d| < ulp(x), as double-doubles (s_hi, s_lo, c_hi, c_lo): d is computed in pieces
    (x - k P1 is exact by Sterbenz, the rest is gathered by two-sums), then sin x = sin(k pi/2) cos d + cos(k pi/2) sin d
    with sin d = d and cos d = 1 - d^2 / 2 (|d| < 2^-36: the next terms are below 2^-70 of them)."""
    kf = k.astype(np.float64)
    hi, lo = x - kf * _PIO2[0], np.zeros_like(x)
    for p in _PIO2[1:]:
        hi, e = two_sum(hi, -(kf * p))
        lo = lo + e
    dh, dl = two_sum(hi, lo)
    one_lo = -(dh * dh) / 2
    r = k.astype(np.int64) & 3
    sk, ck = np.array([0.0, 1.0, 0.0, -1.0])[r], np.array([1.0, 0.0, -1.0, 0.0])[r]
    even = r % 2 == 0
    s_hi, s_lo = np.where(even, ck * dh, sk), np.where(even, ck * dl, sk * one_lo)
    c_hi, c_lo = np.where(even, ck, -sk * dh), np.where(even, ck * one_lo, -sk * dl)
    return s_hi, s_lo, c_hi, c_lo


def kgrid_inputs(fix) -> tuple:
    """(k, x) of the doubles next to k pi/2 on both sides, from the fixture's compact form."""
    k = np.arange(1, fix["sincos_kgrid_n"][()] + 1)
    base = (k * (np.pi / 2)).view(np.int64)
    lo = (base + fix["sincos_kgrid_off"].astype(np.int64)).view(np.float64)
    hi = np.nextafter(lo, np.inf)
    return np.concatenate([k, k]), np.concatenate([lo, hi])
