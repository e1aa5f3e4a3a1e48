// jm_deform.h -- the gym_jiminy `DeformationEstimator` observer block as one batched HIP kernel: every lane is one
// environment, arrays are `[rows][B]` like the physics state and the blocks of jm_blocks.h.
//
// Reference (numba / numpy code restated here per lane, scalar branches become per-lane selects or short branches):
//   refresh_observation                   python/gym_jiminy/common/gym_jiminy/common/blocks/deformation_estimator.py:831-863
//   flexibility_estimator                 deformation_estimator.py:139-235
//   _compute_orientation_error            deformation_estimator.py:30-76
//   _compute_deformation_from_deviation   deformation_estimator.py:80-134
// (the quaternion functions of utils/math.py it calls are the shared layer of jm_rotation.h)
// The reference evaluates the forward kinematics of the theoretical (rigid) model with pinocchio and reads frame
// rotations from it (:840-841, :794-800); here every frame of interest is a short list of (constant rotation, joint
// rotation about an axis by an encoder angle) segments, evaluated per lane.  All lanes interpret the same tables: their
// reads are wave-uniform (indexed by loop counters only) and become scalar loads.  The per-lane state is a rotation
// matrix and a few quaternions in registers; a chain is streamed IMU by IMU (the deviation of the previous IMU is the
// only thing carried along), so nothing is indexed at run time.
#pragma once
#include <string>
#include <vector>

#include "jm_rotation.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_chain, offset of the frame directory, offset of the segment ints,
// chain records ...], a chain record = [K, M, M x (imu column, frame), K x (flipped, frame)]; frame directory = per frame
// (first segment, segment count); segment ints and `dt` (float64) = the segments of jm_rotation.h (index = encoder,
// ratio = encoder ratio).
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
    dt.clear();
    pack_segments(d->n_seg, d->seg_kind, d->seg_enc, d->seg_rot, d->seg_axis, d->seg_ratio, it, dt);
    return true;
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
        const double * d = dt + (long long)s * SEG_DOUBLES;
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
    const Quat<T> q = quat_load(imu_quat, it[rec], nB, B, lane);
    const M3<T> R = deform_frame_rot<T>(it, dt, it[rec + 1], enc, B, lane);
    if (ignore_twist)
    {
        const V3<T> v = deform_tilt_error(R, q);
        return swing_from_vector(v.x, v.y, v.z, chain_singular);
    }
    return quat_mul(q, matrix_to_quat(R), T(1), T(-1));
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
                const Quat<T> q = quat_load(imu_quat, it[imu_rec + 2 * i], iB, B, lane);
                const M3<T> R = deform_frame_rot<T>(it, dt, it[imu_rec + 2 * i + 1], enc, B, lane);
                singular |= deform_tilt_error(R, q).z < T(-1) + T(1e-5);
            }
        Quat<T> dev = deform_deviation<T>(it, dt, imu_rec, ignore_twist, singular, enc, imu_quat, iB, B, lane);
        for (int k = 0; k < K; ++k, ++col)
        {
            const Quat<T> qf = matrix_to_quat(deform_frame_rot<T>(it, dt, it[flex_rec + 2 * k + 1], enc, B, lane));
            const Quat<T> parent = quat_mul(dev, qf, T(1), T(1));
            Quat<T> child = qf;     // orphan end: the kinematic flexibility quaternion itself (:123-124)
            if (k + 1 < M)
            {
                dev = deform_deviation<T>(it, dt, imu_rec + 2 * (k + 1), ignore_twist, singular, enc, imu_quat, iB, B, lane);
                child = quat_mul(dev, qf, T(1), T(1));
            }
            Quat<T> e = quat_mul(parent, child, T(-1), T(1));
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
