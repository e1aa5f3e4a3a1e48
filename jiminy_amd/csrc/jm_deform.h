// jm_deform.h -- the gym_jiminy `DeformationEstimator` observer block as one batched HIP kernel: every lane is one
// environment, arrays are `[rows][B]` like the physics state and the blocks of jm_blocks.h.
//
// Reference (numba / numpy code restated here per lane, scalar branches become per-lane selects or short branches):
//   refresh_observation                   python/gym_jiminy/common/gym_jiminy/common/blocks/deformation_estimator.py:831-863
//   flexibility_estimator                 deformation_estimator.py:139-235
//   _compute_orientation_error            deformation_estimator.py:30-76
//   _compute_deformation_from_deviation   deformation_estimator.py:80-134
//   matrices_to_quat                      python/gym_jiminy/common/gym_jiminy/common/utils/math.py:306-360
//   quat_multiply                         utils/math.py:570-626
//   compute_tilt_from_quat                utils/math.py:1045-1060
//   swing_from_vector                     utils/math.py:1066-1133
//   quat_to_rpy                           utils/math.py:158-201
// The reference evaluates the forward kinematics of the theoretical (rigid) model with pinocchio and reads frame
// rotations from it (:840-841, :794-800); here every frame of interest is a short list of (constant rotation, joint
// rotation about an axis by an encoder angle) segments, evaluated per lane.  All lanes interpret the same tables: their
// reads are wave-uniform (indexed by loop counters only) and become scalar loads.  The per-lane state is a rotation
// matrix and a few quaternions in registers; a chain is streamed IMU by IMU (the deviation of the previous IMU is the
// only thing carried along), so nothing is indexed at run time.
//
// One place where the reference's text is undefined: in the singular branch of `swing_from_vector` the flag `esp_ratio`
// is only assigned when exactly one of |v_x|, |v_y| is below 1e-5; when neither is (which needs |v_z + 1| < 1e-5 with
// both components above 1e-5) the general formula of its last branch is used here.
#pragma once
#include <string>
#include <vector>

#include "jm_math.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_chain, offset of the frame directory, offset of the segment ints,
// chain records ...], a chain record = [K, M, M x (imu column, frame), K x (flipped, frame)]; frame directory = per frame
// (first segment, segment count); segment ints = per segment (kind, encoder).  `dt` (float64) = per segment 9 rotation
// entries, 3 axis entries, the encoder ratio.
constexpr int DEFORM_SEG_DOUBLES = 13;
constexpr int DEFORM_MAX_SEGS_PER_FRAME = 64;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool deform_pack(const jm_deform_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    if (!d) { why = "jm_deform_plan_create: null description"; return false; }
    if (!d->chain_nflex || !d->chain_orphan || !d->chain_imu || !d->chain_imu_frame || !d->flex_frame ||
        !d->flex_flipped || !d->frame_seg_start || !d->seg_kind || !d->seg_enc || !d->seg_rot || !d->seg_axis || !d->seg_ratio)
    { why = "jm_deform_plan_create: null array in the description"; return false; }
    if (d->n_imu <= 0 || d->n_enc < 0 || d->n_chain <= 0 || d->n_frame <= 0 || d->n_seg <= 0)
    { why = "jm_deform_plan_create: bad sizes"; return false; }
    if (d->n_flex <= 0) { why = "Please specify at least one IMU and one deformation point."; return false; }
    if (d->frame_seg_start[0] != 0 || d->frame_seg_start[d->n_frame] != d->n_seg)
    { why = "jm_deform_plan_create: frame_seg_start must run from 0 to n_seg"; return false; }
    for (int f = 0; f < d->n_frame; ++f)
    {
        const int n = d->frame_seg_start[f + 1] - d->frame_seg_start[f];
        if (n <= 0 || n > DEFORM_MAX_SEGS_PER_FRAME)
        { why = "jm_deform_plan_create: frame " + std::to_string(f) + " has a bad segment count"; return false; }
    }
    for (int s = 0; s < d->n_seg; ++s)
    {
        if (d->seg_kind[s] < 0 || d->seg_kind[s] > 4)
        { why = "jm_deform_plan_create: segment " + std::to_string(s) + " has an unknown joint kind"; return false; }
        if (d->seg_kind[s] != 0 && (d->seg_enc[s] < 0 || d->seg_enc[s] >= d->n_enc))
        { why = "jm_deform_plan_create: segment " + std::to_string(s) + " names encoder " + std::to_string(d->seg_enc[s]) +
                " out of range [0, " + std::to_string(d->n_enc) + ")"; return false; }
    }
    int n_flex = 0, n_imu = 0;
    for (int c = 0; c < d->n_chain; ++c)
    {
        if (d->chain_nflex[c] <= 0) { why = "jm_deform_plan_create: chain " + std::to_string(c) + " has no flexibility point"; return false; }
        if (d->chain_orphan[2 * c])
        { why = "jm_deform_plan_create: chain " + std::to_string(c) + " misses its first IMU: not supported (nor by the reference's block)"; return false; }
        n_flex += d->chain_nflex[c];
        n_imu += d->chain_nflex[c] + 1 - (d->chain_orphan[2 * c + 1] ? 1 : 0);
    }
    if (n_flex != d->n_flex) { why = "jm_deform_plan_create: n_flex is not the sum of chain_nflex"; return false; }
    for (int i = 0; i < n_imu; ++i)
    {
        if (d->chain_imu[i] < 0 || d->chain_imu[i] >= d->n_imu)
        { why = "jm_deform_plan_create: IMU index " + std::to_string(d->chain_imu[i]) + " out of range [0, " + std::to_string(d->n_imu) + ")"; return false; }
        if (d->chain_imu_frame[i] < 0 || d->chain_imu_frame[i] >= d->n_frame)
        { why = "jm_deform_plan_create: IMU frame out of range"; return false; }
    }
    for (int k = 0; k < n_flex; ++k)
        if (d->flex_frame[k] < 0 || d->flex_frame[k] >= d->n_frame)
        { why = "jm_deform_plan_create: flexibility frame out of range"; return false; }

    it.clear();
    it.push_back(d->n_chain);
    it.push_back(0);
    it.push_back(0);
    int ci = 0, cf = 0;
    for (int c = 0; c < d->n_chain; ++c)
    {
        const int K = d->chain_nflex[c], M = K + 1 - (d->chain_orphan[2 * c + 1] ? 1 : 0);
        it.push_back(K);
        it.push_back(M);
        for (int i = 0; i < M; ++i, ++ci) { it.push_back(d->chain_imu[ci]); it.push_back(d->chain_imu_frame[ci]); }
        for (int k = 0; k < K; ++k, ++cf) { it.push_back(d->flex_flipped[cf] ? 1 : 0); it.push_back(d->flex_frame[cf]); }
    }
    it[1] = (int32_t)it.size();
    for (int f = 0; f < d->n_frame; ++f)
    {
        it.push_back(d->frame_seg_start[f]);
        it.push_back(d->frame_seg_start[f + 1] - d->frame_seg_start[f]);
    }
    it[2] = (int32_t)it.size();
    for (int s = 0; s < d->n_seg; ++s) { it.push_back(d->seg_kind[s]); it.push_back(d->seg_kind[s] ? d->seg_enc[s] : 0); }
    dt.assign((size_t)d->n_seg * DEFORM_SEG_DOUBLES, 0.0);
    for (int s = 0; s < d->n_seg; ++s)
    {
        double * o = dt.data() + (size_t)s * DEFORM_SEG_DOUBLES;
        for (int k = 0; k < 9; ++k) o[k] = d->seg_rot[9 * s + k];
        for (int k = 0; k < 3; ++k) o[9 + k] = d->seg_axis[3 * s + k];
        o[12] = d->seg_ratio[s];
    }
    return true;
}

template<class T> struct Quat
{
    T x, y, z, w;
};

// `quat_multiply` (utils/math.py:611-622): sl / sr = -1 conjugates the left / right factor
template<class T> JM_DEV Quat<T> deform_qmul(const Quat<T> & l, const Quat<T> & r, T sl, T sr)
{
    return {sl * l.w * r.x + l.x * sr * r.w + l.y * r.z - l.z * r.y,
            sl * l.w * r.y - l.x * r.z + l.y * sr * r.w + l.z * r.x,
            sl * l.w * r.z + l.x * r.y - l.y * r.x + l.z * sr * r.w,
            sl * l.w * sr * r.w - l.x * r.x - l.y * r.y - l.z * r.z};
}

// `matrices_to_quat` (utils/math.py:327-356), one matrix
template<class T> JM_DEV Quat<T> deform_mat_to_quat(const M3<T> & m)
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
template<class T> JM_DEV Quat<T> deform_renorm(const Quat<T> & q)
{
    const T k = (T(3) - (q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w)) / T(2);
    return {q.x * k, q.y * k, q.z * k, q.w * k};
}

// `swing_from_vector` (utils/math.py:1080-1133) for one IMU of a chain.  `chain_singular`: some IMU of the chain is below
// the singular threshold -- the reference then goes IMU by IMU (each normalised by its scalar call) and normalises the
// whole chain once more.
template<class T> JM_DEV Quat<T> deform_swing(T vx, T vy, T vz, bool chain_singular)
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
    q = deform_renorm(q);
    if (chain_singular) q = deform_renorm(q);
    return q;
}

// rotation of frame `frame` of the theoretical model: product of its segments
template<class T>
JM_DEV M3<T> deform_frame_rot(const int32_t * __restrict__ it, const double * __restrict__ dt, int frame,
                              const T * __restrict__ enc, long long B, long long lane)
{
    const int fd = it[1] + 2 * frame, si = it[2];
    const int s0 = it[fd], s1 = s0 + it[fd + 1];
    M3<T> R = ident3<T>();
    for (int s = s0; s < s1; ++s)
    {
        const double * d = dt + (long long)s * DEFORM_SEG_DOUBLES;
        const M3<T> Cm = {(T)d[0], (T)d[1], (T)d[2], (T)d[3], (T)d[4], (T)d[5], (T)d[6], (T)d[7], (T)d[8]};
        R = s == s0 ? Cm : R * Cm;
        const int kind = it[si + 2 * s];
        if (kind != 0)
        {
            const T angle = enc[(long long)it[si + 2 * s + 1] * 2 * B + lane] * (T)d[12];
            T sn, cs;
            sincos_(angle, &sn, &cs);
            const M3<T> J = kind <= 3 ? rot_axis<T>(kind - 1, cs, sn) : rot_rodrigues<T>(v3((T)d[9], (T)d[10], (T)d[11]), cs, sn);
            R = R * J;
        }
    }
    return R;
}

template<class T>
JM_DEV Quat<T> deform_load_quat(const T * __restrict__ imu_quat, int col, long long nB, long long B, long long lane)
{
    const long long o = (long long)col * B + lane;
    return {imu_quat[o], imu_quat[nB + o], imu_quat[2 * nB + o], imu_quat[3 * nB + o]};
}

// tilt error of one IMU in the world frame: R_kin (R_obs^T e_z)   (deformation_estimator.py:55-63)
template<class T> JM_DEV V3<T> deform_tilt_error(const M3<T> & R, const Quat<T> & q)
{
    const V3<T> tilt = {T(2) * (q.x * q.z - q.y * q.w), T(2) * (q.y * q.z + q.w * q.x), T(1) - T(2) * (q.x * q.x + q.y * q.y)};
    return R * tilt;
}

// deviation of IMU record `rec` (imu column, frame) from its kinematic orientation (`_compute_orientation_error`)
template<class T>
JM_DEV Quat<T> deform_deviation(const int32_t * __restrict__ it, const double * __restrict__ dt, int rec, bool ignore_twist,
                                bool chain_singular, const T * __restrict__ enc, const T * __restrict__ imu_quat, long long nB,
                                long long B, long long lane)
{
    const Quat<T> q = deform_load_quat(imu_quat, it[rec], nB, B, lane);
    const M3<T> R = deform_frame_rot<T>(it, dt, it[rec + 1], enc, B, lane);
    if (ignore_twist)
    {
        const V3<T> v = deform_tilt_error(R, q);
        return deform_swing(v.x, v.y, v.z, chain_singular);
    }
    return deform_qmul(q, deform_mat_to_quat(R), T(1), T(-1));
}

// The block for one lane.  encoder `[n_enc][2][B]`, imu_quat `[4][n_imu][B]`, out_quat `[4][n_flex][B]`, out_rpy
// `[3][n_flex][B]` or null.
template<class T>
JM_DEV void deform_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, int n_imu, int n_flex, int ignore_twist_,
                        const T * __restrict__ enc, const T * __restrict__ imu_quat, T * __restrict__ out_quat,
                        T * __restrict__ out_rpy, long long B, long long lane)
{
    const bool ignore_twist = ignore_twist_ != 0;
    const long long iB = (long long)n_imu * B, fB = (long long)n_flex * B;
    const int n_chain = it[0];
    int c = 3, col = 0;
    for (int chain = 0; chain < n_chain; ++chain)
    {
        const int K = it[c], M = it[c + 1], imu_rec = c + 2, flex_rec = imu_rec + 2 * M;
        bool singular = false;
        if (ignore_twist)
            for (int i = 0; i < M; ++i)
            {
                const Quat<T> q = deform_load_quat(imu_quat, it[imu_rec + 2 * i], iB, B, lane);
                const M3<T> R = deform_frame_rot<T>(it, dt, it[imu_rec + 2 * i + 1], enc, B, lane);
                singular |= deform_tilt_error(R, q).z < T(-1) + T(1e-5);
            }
        Quat<T> dev = deform_deviation<T>(it, dt, imu_rec, ignore_twist, singular, enc, imu_quat, iB, B, lane);
        for (int k = 0; k < K; ++k, ++col)
        {
            const Quat<T> qf = deform_mat_to_quat(deform_frame_rot<T>(it, dt, it[flex_rec + 2 * k + 1], enc, B, lane));
            const Quat<T> parent = deform_qmul(dev, qf, T(1), T(1));
            Quat<T> child = qf;     // orphan end: the kinematic flexibility quaternion itself (:123-124)
            if (k + 1 < M)
            {
                dev = deform_deviation<T>(it, dt, imu_rec + 2 * (k + 1), ignore_twist, singular, enc, imu_quat, iB, B, lane);
                child = deform_qmul(dev, qf, T(1), T(1));
            }
            Quat<T> e = deform_qmul(parent, child, T(-1), T(1));
            if (it[flex_rec + 2 * k]) e.w = -e.w;
            const long long o = (long long)col * B + lane;
            out_quat[o] = e.x; out_quat[fB + o] = e.y; out_quat[2 * fB + o] = e.z; out_quat[3 * fB + o] = e.w;
            if (out_rpy)
            {
                // `quat_to_rpy` (utils/math.py:182-197)
                const T xx = e.x * e.x, xy = e.x * e.y, xw = e.x * e.w;
                const T yy = e.y * e.y, yz = e.y * e.z, zz = e.z * e.z, zw = e.z * e.w, ww = e.w * e.w;
                const T n2 = (T(3) - (xx + yy + zz + ww)) / T(2);
                const T yw = e.y * e.w * n2, xz = e.x * e.z * n2;
                out_rpy[o] = atan2_(T(2) * (xw + yz), T(1) - T(2) * (xx + yy));
                out_rpy[fB + o] = -T(3.14159265358979323846) / T(2) +
                                  T(2) * atan2_(sqrt_(T(1) + T(2) * (yw - xz)), sqrt_(T(1) - T(2) * (yw - xz)));
                out_rpy[2 * fB + o] = atan2_(T(2) * (zw + xy), T(1) - T(2) * (yy + zz));
            }
        }
        c = flex_rec + 2 * K;
    }
}

#ifndef JM_HOST_EMU
struct DeformArgs
{
    const int32_t * it;
    const double * dt;
    int n_imu, n_flex, ignore_twist;
};
template<class T>
__global__ void __launch_bounds__(256) k_deformation_estimator(const DeformArgs p, const T * __restrict__ enc,
                                                                const T * __restrict__ imu_quat, T * __restrict__ out_quat,
                                                                T * __restrict__ out_rpy, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    deform_lane<T>(p.it, p.dt, p.n_imu, p.n_flex, p.ignore_twist, enc, imu_quat, out_quat, out_rpy, B, lane);
}
#endif
}  // namespace jm
