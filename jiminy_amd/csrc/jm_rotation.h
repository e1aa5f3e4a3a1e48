// jm_rotation.h -- the rotation / quaternion layer the observer blocks share (jm_deform.h, jm_attitude.h): per-lane functions
// over quaternions xyzw in registers, arrays `[rows][B]`, and the record a frame's rotation segments are packed in.
//
// Reference (numba / numpy code of python/gym_jiminy/common/gym_jiminy/common/utils/math.py restated per lane):
//   matrices_to_quat         :306-360
//   quat_multiply            :570-626
//   compute_tilt_from_quat   :1045-1060
//   swing_from_vector        :1066-1133
//   quat_to_rpy              :158-201
//
// One place where the reference's text is undefined: in the singular branch of `swing_from_vector` the flag `esp_ratio`
// is only assigned when exactly one of |v_x|, |v_y| is below 1e-5; when neither is (which needs |v_z + 1| < 1e-5 with
// both components above 1e-5) the general formula of its last branch is used here.
#pragma once
#include <cstdint>
#include <vector>

#include "jm_math.h"

namespace jm
{
template<class T> struct Quat
{
    T x, y, z, w;
};

// `quat_multiply` (utils/math.py:611-622): sl / sr = -1 conjugates the left / right factor
template<class T> JM_DEV Quat<T> quat_mul(const Quat<T> & l, const Quat<T> & r, T sl, T sr)
{
    return {sl * l.w * r.x + l.x * sr * r.w + l.y * r.z - l.z * r.y,
            sl * l.w * r.y - l.x * r.z + l.y * sr * r.w + l.z * r.x,
            sl * l.w * r.z + l.x * r.y - l.y * r.x + l.z * sr * r.w,
            sl * l.w * sr * r.w - l.x * r.x - l.y * r.y - l.z * r.z};
}

// `matrices_to_quat` (utils/math.py:327-356), one matrix
template<class T> JM_DEV Quat<T> matrix_to_quat(const M3<T> & m)
{
    T t, x, y, z, w;
    if (m.m22 < T(0))
    {
        if (m.m00 > m.m11) { t = T(1) + m.m00 - m.m11 - m.m22; x = t; y = m.m10 + m.m01; z = m.m02 + m.m20; w = m.m21 - m.m12; }
        else { t = T(1) - m.m00 + m.m11 - m.m22; x = m.m10 + m.m01; y = t; z = m.m21 + m.m12; w = m.m02 - m.m20; }
    }
    else
    {
        if (m.m00 < -m.m11) { t = T(1) - m.m00 - m.m11 + m.m22; x = m.m02 + m.m20; y = m.m21 + m.m12; z = t; w = m.m10 - m.m01; }
        else { t = T(1) + m.m00 + m.m11 + m.m22; x = m.m21 - m.m12; y = m.m02 - m.m20; z = m.m10 - m.m01; w = t; }
    }
    const T n = T(2) * sqrt_(t);
    return {x / n, y / n, z / n, w / n};
}

// first-order normalisation `q *= (3 - |q|^2) / 2` (utils/math.py:1133)
template<class T> JM_DEV Quat<T> quat_renorm(const Quat<T> & q)
{
    const T k = (T(3) - (q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w)) / T(2);
    return {q.x * k, q.y * k, q.z * k, q.w * k};
}

// `swing_from_vector` (utils/math.py:1080-1133) for one vector of a group (the IMUs of a chain, the IMUs of an
// environment).  `any_singular`: some vector of the group is below the singular threshold -- the reference decides its
// branch with `np.any` over the group, then goes vector by vector (each normalised by its scalar call) and normalises the
// whole group once more.
template<class T> JM_DEV Quat<T> swing_from_vector(T vx, T vy, T vz, bool any_singular)
{
    const T thr = T(1e-5);
    Quat<T> q;
    if (vz < T(-1) + thr)
    {
        const T eps_thr = sqrt_(thr);
        const bool eps_x = -thr < vx && vx < thr, eps_y = -thr < vy && vy < thr;
        T ratio = T(0);
        bool eps_ratio = false;
        if (eps_x && !eps_y) { ratio = vx / vy; eps_ratio = -eps_thr < ratio && ratio < eps_thr; }
        else if (eps_y && !eps_x) { ratio = vy / vx; eps_ratio = -eps_thr < ratio && ratio < eps_thr; }
        const T w_2 = (T(1) + fmax_(vz, T(-1))) / T(2);
        const T sw = sqrt_(T(1) - w_2);
        if (eps_x && eps_y) { q.x = T(0); q.y = sw; }
        else if (eps_ratio && eps_x) { q.x = -sw * (T(1) - T(0.5) * ratio * ratio); q.y = sw * (ratio - T(0.5) * ratio * ratio * ratio); }
        else if (eps_ratio && eps_y) { q.x = -sw * (ratio - T(0.5) * ratio * ratio * ratio); q.y = sw * (T(1) - T(0.5) * ratio * ratio); }
        else
        {
            const T rxy = vx / vy, ryx = vy / vx;
            q.x = -sqrt_((T(1) - w_2) / (T(1) + rxy * rxy));
            q.y = sqrt_((T(1) - w_2) / (T(1) + ryx * ryx));
        }
        q.z = T(0);
        q.w = sqrt_(w_2);
    }
    else
    {
        const T s = sqrt_(T(2) * (T(1) + vz));
        q = {vy / s, -vx / s, T(0), s / T(2)};
    }
    q = quat_renorm(q);
    if (any_singular) q = quat_renorm(q);
    return q;
}

// quaternion `col` of an array `[4][n][B]` (nB = n * B)
template<class T> JM_DEV Quat<T> quat_load(const T * __restrict__ quat, int col, long long nB, long long B, long long lane)
{
    const long long o = (long long)col * B + lane;
    return {quat[o], quat[nB + o], quat[2 * nB + o], quat[3 * nB + o]};
}
template<class T> JM_DEV void quat_store(T * __restrict__ quat, long long nB, long long o, const Quat<T> & q)
{
    quat[o] = q.x; quat[nB + o] = q.y; quat[2 * nB + o] = q.z; quat[3 * nB + o] = q.w;
}

// `quat_to_rpy` (utils/math.py:182-197) into an array `[3][n][B]`
template<class T> JM_DEV void quat_store_rpy(T * __restrict__ rpy, long long nB, long long o, const Quat<T> & e)
{
    const T xx = e.x * e.x, xy = e.x * e.y, xw = e.x * e.w;
    const T yy = e.y * e.y, yz = e.y * e.z, zz = e.z * e.z, zw = e.z * e.w, ww = e.w * e.w;
    const T n2 = (T(3) - (xx + yy + zz + ww)) / T(2);
    const T yw = e.y * e.w * n2, xz = e.x * e.z * n2;
    rpy[o] = atan2_(T(2) * (xw + yz), T(1) - T(2) * (xx + yy));
    rpy[nB + o] = -T(3.14159265358979323846) / T(2) + T(2) * atan2_(sqrt_(T(1) + T(2) * (yw - xz)), sqrt_(T(1) - T(2) * (yw - xz)));
    rpy[2 * nB + o] = atan2_(T(2) * (zw + xy), T(1) - T(2) * (yy + zz));
}

// `compute_tilt_from_quat` (utils/math.py:1056-1059): R(q)^T e_z, in one of two arithmetic forms chosen at compile time.
//   TILT_FUSED    as the compiler contracts it under the library's -ffp-contract=fast (products fused into the sums):
//                 the plain Mahony function and the DeformationEstimator.
//   TILT_ROUNDED  the three lines evaluated as written, every product rounded on its own: the attitude observers, where
//                 the tilt feeds the singular branch of `swing_from_vector` and one ulp of v_z is amplified by 1e5.  Under
//                 -ffp-contract=fast the backend fuses a multiply into the following add whatever a pragma says; passing
//                 each product through an empty asm statement keeps it a value of its own (no instruction is emitted).
enum TiltForm { TILT_FUSED, TILT_ROUNDED };
template<TiltForm F, class T> JM_DEV T tilt_product(T x)
{
#ifndef JM_HOST_EMU
    if constexpr (F == TILT_ROUNDED) asm volatile("" : "+v"(x));
#endif
    return x;
}
template<TiltForm F, class T> JM_DEV V3<T> quat_tilt(const Quat<T> & q)
{
    const T xz = tilt_product<F>(q.x * q.z), yw = tilt_product<F>(q.y * q.w);
    const T yz = tilt_product<F>(q.y * q.z), wx = tilt_product<F>(q.w * q.x);
    const T xx = tilt_product<F>(q.x * q.x), yy = tilt_product<F>(q.y * q.y);
    return {T(2) * (xz - yw), T(2) * (yz + wx), T(1) - T(2) * (xx + yy)};
}

// ---- rotation of a frame as a product of segments: a constant rotation, then the rotation of one joint.  A segment is
// two ints (kind, index of what the joint rotation is read from) and SEG_DOUBLES doubles (9 rotation entries row-major,
// 3 axis entries, one ratio).  All lanes interpret the same tables: their reads are wave-uniform (indexed by loop counters
// only) and become scalar loads.
constexpr int SEG_DOUBLES = 13;
constexpr int SEG_NONE = 0, SEG_AXIS = 4, SEG_UNBOUNDED = 5, SEG_QUAT = 6;   // (1..3: about x, y, z)

// host: append the packed segments of a description to its plan
inline void pack_segments(int n_seg, const int32_t * kind, const int32_t * index, const double * rot, const double * axis,
                          const double * ratio, std::vector<int32_t> & it, std::vector<double> & dt)
{
    for (int s = 0; s < n_seg; ++s)
    {
        it.push_back(kind[s]);
        it.push_back(kind[s] ? index[s] : 0);
        dt.insert(dt.end(), rot + 9 * s, rot + 9 * s + 9);
        dt.insert(dt.end(), axis + 3 * s, axis + 3 * s + 3);
        dt.push_back(ratio ? ratio[s] : 0.0);
    }
}
}  // namespace jm
