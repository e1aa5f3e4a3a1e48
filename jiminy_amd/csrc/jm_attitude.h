// jm_attitude.h -- the attitude observers of gym_jiminy as batched HIP kernels: what the `MahonyFilter` class does around
// its numba function (per-IMU gains, twist removal, Euler angles, initialisation at the first refresh of an episode) and
// the `BodyObserver` block.  Every lane is one environment, arrays are `[rows][B]` like the physics state and the blocks
// of jm_blocks.h / jm_deform.h, whose per-lane functions (`deform_swing`, `deform_mat_to_quat`, `deform_qmul`) are used here.
//
// Reference (numba / numpy code restated here per lane):
//   MahonyFilter.refresh_observation   python/gym_jiminy/common/gym_jiminy/common/blocks/mahony_filter.py:337-393
//   mahony_filter                      mahony_filter.py:28-101
//   BodyObserver.refresh_observation   python/gym_jiminy/common/gym_jiminy/common/blocks/body_orientation_observer.py:237-266
//   update_twist                       body_orientation_observer.py:26-71
//   remove_twist_from_quat             python/gym_jiminy/common/gym_jiminy/common/utils/math.py:1202-1244
//   compute_tilt_from_quat             utils/math.py:1045-1060
//   swing_from_vector                  utils/math.py:1066-1133
//   quat_multiply / quat_apply         utils/math.py:570-626 / 645-709
//   matrices_to_quat / quat_to_rpy     utils/math.py:306-360 / 158-201
// `swing_from_vector` on the IMUs of one environment decides its singular branch with `np.any` over them: the flag handed to
// `deform_swing` is "any IMU of the lane" (jm_deform.h: each IMU then takes the scalar branch and is normalised twice).  The
// undefined `esp_ratio` case is handled as documented at the top of jm_deform.h.
//
// The true IMU orientations of the exact initialisation (the reference reads `oMf` of pinocchio, :357-366) are a
// rotation-only walk from the root to the sensor frame over the lane's `q` rows: per IMU a list of segments (constant
// rotation, then a joint rotation read from `q`).  All lanes interpret the same tables: their reads are indexed by loop
// counters only and become scalar loads; per-lane state is one rotation matrix and one quaternion in registers.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "jm_deform.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_imu, offset of the segment ints, n_imu x (first segment, segment count),
// n_seg x (kind, q index)]; `dt` (float64) = n_imu x (kp, ki, rel_quat xyzw), then per segment 9 rotation entries and 3
// axis entries.
constexpr int ATT_IMU_DOUBLES = 6;
constexpr int ATT_SEG_DOUBLES = 12;
constexpr int ATT_MAX_SEGS_PER_IMU = 256;
constexpr int ATT_SEG_NONE = 0, ATT_SEG_AXIS = 4, ATT_SEG_UNBOUNDED = 5, ATT_SEG_QUAT = 6;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool attitude_pack(const jm_attitude_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    if (!d) { why = "jm_attitude_plan_create: null description"; return false; }
    if (!d->kp || !d->ki || !d->rel_quat || !d->frame_seg_start || !d->seg_kind || !d->seg_q_index || !d->seg_rot || !d->seg_axis)
    { why = "jm_attitude_plan_create: null array in the description"; return false; }
    if (d->n_imu <= 0 || d->n_seg <= 0 || d->nq < 0) { why = "jm_attitude_plan_create: bad sizes"; return false; }
    if (d->frame_seg_start[0] != 0 || d->frame_seg_start[d->n_imu] != d->n_seg)
    { why = "jm_attitude_plan_create: frame_seg_start must run from 0 to n_seg"; return false; }
    for (int s = 0; s < d->n_imu; ++s)
    {
        const int n = d->frame_seg_start[s + 1] - d->frame_seg_start[s];
        if (n <= 0 || n > ATT_MAX_SEGS_PER_IMU)
        { why = "jm_attitude_plan_create: IMU " + std::to_string(s) + " has a bad segment count"; return false; }
        if (!std::isfinite(d->kp[s]) || !std::isfinite(d->ki[s]))
        { why = "jm_attitude_plan_create: IMU " + std::to_string(s) + " has a gain that is not finite"; return false; }
        double n2 = 0.0;
        for (int k = 0; k < 4; ++k) n2 += d->rel_quat[4 * s + k] * d->rel_quat[4 * s + k];
        if (!(std::fabs(n2 - 1.0) <= 1e-6))
        { why = "jm_attitude_plan_create: rel_quat of IMU " + std::to_string(s) + " is not a unit quaternion"; return false; }
    }
    for (int s = 0; s < d->n_seg; ++s)
    {
        const int kind = d->seg_kind[s], qi = d->seg_q_index[s];
        if (kind < 0 || kind > ATT_SEG_QUAT)
        { why = "jm_attitude_plan_create: segment " + std::to_string(s) + " has an unknown joint kind"; return false; }
        const int rows = kind == ATT_SEG_NONE ? 0 : (kind == ATT_SEG_QUAT ? 4 : (kind == ATT_SEG_UNBOUNDED ? 2 : 1));
        if (rows && (qi < 0 || qi + rows > d->nq))
        { why = "jm_attitude_plan_create: segment " + std::to_string(s) + " reads q rows [" + std::to_string(qi) + ", " +
                std::to_string(qi + rows) + ") out of range [0, " + std::to_string(d->nq) + ")"; return false; }
    }
    it.clear();
    it.push_back(d->n_imu);
    it.push_back(2 + 2 * d->n_imu);
    for (int s = 0; s < d->n_imu; ++s)
    {
        it.push_back(d->frame_seg_start[s]);
        it.push_back(d->frame_seg_start[s + 1] - d->frame_seg_start[s]);
    }
    for (int s = 0; s < d->n_seg; ++s) { it.push_back(d->seg_kind[s]); it.push_back(d->seg_kind[s] ? d->seg_q_index[s] : 0); }
    dt.assign((size_t)d->n_imu * ATT_IMU_DOUBLES + (size_t)d->n_seg * ATT_SEG_DOUBLES, 0.0);
    for (int s = 0; s < d->n_imu; ++s)
    {
        double * o = dt.data() + (size_t)s * ATT_IMU_DOUBLES;
        o[0] = d->kp[s];
        o[1] = d->ki[s];
        for (int k = 0; k < 4; ++k) o[2 + k] = d->rel_quat[4 * s + k];
    }
    for (int s = 0; s < d->n_seg; ++s)
    {
        double * o = dt.data() + (size_t)d->n_imu * ATT_IMU_DOUBLES + (size_t)s * ATT_SEG_DOUBLES;
        for (int k = 0; k < 9; ++k) o[k] = d->seg_rot[9 * s + k];
        for (int k = 0; k < 3; ++k) o[9 + k] = d->seg_axis[3 * s + k];
    }
    return true;
}

// `compute_tilt_from_quat` (utils/math.py:1056-1059).  Near the singular branch of `swing_from_vector` one ulp of v_z is
// amplified by 1e5, so the three lines are evaluated as written: every product is rounded on its own.  The library is
// built with -ffp-contract=fast, under which the backend fuses a multiply into the following add whatever a pragma says;
// passing each product through an empty asm statement keeps it a value of its own (no instruction is emitted for it).
template<class T> JM_DEV T attitude_rounded(T x)
{
#ifndef JM_HOST_EMU
    asm volatile("" : "+v"(x));
#endif
    return x;
}
template<class T> JM_DEV V3<T> attitude_tilt(const Quat<T> & q)
{
    const T xz = attitude_rounded(q.x * q.z), yw = attitude_rounded(q.y * q.w);
    const T yz = attitude_rounded(q.y * q.z), wx = attitude_rounded(q.w * q.x);
    const T xx = attitude_rounded(q.x * q.x), yy = attitude_rounded(q.y * q.y);
    return {T(2) * (xz - yw), T(2) * (yz + wx), T(1) - T(2) * (xx + yy)};
}

template<class T> JM_DEV void attitude_store_quat(T * __restrict__ quat, long long nB, long long o, const Quat<T> & q)
{
    quat[o] = q.x; quat[nB + o] = q.y; quat[2 * nB + o] = q.z; quat[3 * nB + o] = q.w;
}

// `quat_to_rpy` (utils/math.py:182-197)
template<class T> JM_DEV void attitude_store_rpy(T * __restrict__ rpy, long long nB, long long o, const Quat<T> & e)
{
    const T xx = e.x * e.x, xy = e.x * e.y, xw = e.x * e.w;
    const T yy = e.y * e.y, yz = e.y * e.z, zz = e.z * e.z, zw = e.z * e.w, ww = e.w * e.w;
    const T n2 = (T(3) - (xx + yy + zz + ww)) / T(2);
    const T yw = e.y * e.w * n2, xz = e.x * e.z * n2;
    rpy[o] = atan2_(T(2) * (xw + yz), T(1) - T(2) * (xx + yy));
    rpy[nB + o] = -T(3.14159265358979323846) / T(2) + T(2) * atan2_(sqrt_(T(1) + T(2) * (yw - xz)), sqrt_(T(1) - T(2) * (yw - xz)));
    rpy[2 * nB + o] = atan2_(T(2) * (zw + xy), T(1) - T(2) * (yy + zz));
}

// `remove_twist_from_quat` over the IMUs of one lane (in place in `quat`), then `quat_to_rpy` when `rpy` is given; with
// `remove_twist` false only the Euler angles.
template<class T>
JM_DEV void attitude_swing_and_rpy(int n_imu, bool remove_twist, T * __restrict__ quat, T * __restrict__ rpy, long long B, long long lane)
{
    const long long nB = (long long)n_imu * B;
    bool singular = false;
    if (remove_twist)
        for (int s = 0; s < n_imu; ++s)
            singular |= attitude_tilt(deform_load_quat(quat, s, nB, B, lane)).z < T(-1) + T(1e-5);
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        Quat<T> q = deform_load_quat(quat, s, nB, B, lane);
        if (remove_twist)
        {
            const V3<T> v = attitude_tilt(q);
            q = deform_swing(v.x, v.y, v.z, singular);
            attitude_store_quat(quat, nB, o, q);
        }
        if (rpy) attitude_store_rpy(rpy, nB, o, q);
    }
}

// world rotation of the frame of IMU `s`: product of its segments over the lane's `q` rows
template<class T>
JM_DEV M3<T> attitude_frame_rot(const int32_t * __restrict__ it, const double * __restrict__ dt, int s_imu, const T * __restrict__ q,
                                long long B, long long lane)
{
    const int n_imu = it[0], si = it[1];
    const int s0 = it[2 + 2 * s_imu], s1 = s0 + it[3 + 2 * s_imu];
    const double * seg = dt + (long long)n_imu * ATT_IMU_DOUBLES;
    M3<T> R = ident3<T>();
    for (int s = s0; s < s1; ++s)
    {
        const double * d = seg + (long long)s * ATT_SEG_DOUBLES;
        const M3<T> Cm = {(T)d[0], (T)d[1], (T)d[2], (T)d[3], (T)d[4], (T)d[5], (T)d[6], (T)d[7], (T)d[8]};
        R = s == s0 ? Cm : R * Cm;
        const int kind = it[si + 2 * s];
        if (kind == ATT_SEG_NONE) continue;
        const T * qr = q + (long long)it[si + 2 * s + 1] * B + lane;
        M3<T> J;
        if (kind == ATT_SEG_QUAT) J = quat_to_matrix<T>(qr[0], qr[B], qr[2 * B], qr[3 * B]);
        else if (kind == ATT_SEG_UNBOUNDED) J = rot_rodrigues<T>(v3((T)d[9], (T)d[10], (T)d[11]), qr[0], qr[B]);
        else
        {
            T sn, cs;
            sincos_(qr[0], &sn, &cs);
            J = kind <= 3 ? rot_axis<T>(kind - 1, cs, sn) : rot_rodrigues<T>(v3((T)d[9], (T)d[10], (T)d[11]), cs, sn);
        }
        R = R * J;
    }
    return R;
}

// `MahonyFilter.refresh_observation` while `_is_initialized` is false (mahony_filter.py:340-374) for one lane.
// q `[nq][B]`; imu raw field `[n_imu][6][B]`; quat `[4][n_imu][B]`; omega, cf, bias, rpy `[3][n_imu][B]`; twist `[n_imu][B]`.
template<class T>
JM_DEV void attitude_init_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, int n_imu, int exact_init,
                               const T * __restrict__ q, const T * __restrict__ imu, T * __restrict__ quat, T * __restrict__ omega,
                               T * __restrict__ cf, T * __restrict__ bias, T * __restrict__ twist, T * __restrict__ rpy, long long B,
                               long long lane)
{
    const long long nB = (long long)n_imu * B;
    bool exact = exact_init != 0;
    if (!exact)
    {
        // free fall: every component of every accelerometer below 0.1 g (:342)
        const T low = T(0.1 * 9.81);
        bool falling = true;
        for (int s = 0; s < n_imu; ++s)
        {
            const T * g = imu + (long long)s * 6 * B + lane;
            for (int k = 3; k < 6; ++k)
            {
                const T a = g[k * B];
                falling &= (a < T(0) ? -a : a) < low;
            }
        }
        exact = falling;
    }
    bool singular = false;
    if (!exact)
        for (int s = 0; s < n_imu; ++s)
        {
            const T * g = imu + (long long)s * 6 * B + lane;
            const T ax = g[3 * B], ay = g[4 * B], az = g[5 * B];
            singular |= az / sqrt_(ax * ax + ay * ay + az * az) < T(-1) + T(1e-5);
        }
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        Quat<T> e;
        if (exact) e = deform_mat_to_quat(attitude_frame_rot<T>(it, dt, s, q, B, lane));
        else
        {
            const T * g = imu + (long long)s * 6 * B + lane;
            const T ax = g[3 * B], ay = g[4 * B], az = g[5 * B];
            const T n = sqrt_(ax * ax + ay * ay + az * az);
            e = deform_swing(ax / n, ay / n, az / n, singular);
        }
        attitude_store_quat(quat, nB, o, e);
        omega[o] = T(0); omega[nB + o] = T(0); omega[2 * nB + o] = T(0);
        cf[o] = T(0); cf[nB + o] = T(0); cf[2 * nB + o] = T(0);
        bias[o] = T(0); bias[nB + o] = T(0); bias[2 * nB + o] = T(0);
        if (twist) twist[o] = T(0);
        if (rpy) attitude_store_rpy(rpy, nB, o, e);
    }
}

// One tick of an initialised `MahonyFilter` (mahony_filter.py:376-393) for one lane: `mahony_filter` with the gains of
// every IMU, then the twist removal and the Euler angles -- which run after the filter's early return as well.
template<class T>
JM_DEV void mahony_observer_lane(const double * __restrict__ dt, int n_imu, const T * __restrict__ imu, T * __restrict__ quat,
                                 T * __restrict__ omega, T * __restrict__ cf, T * __restrict__ bias, T step, int ignore_twist,
                                 T * __restrict__ rpy, long long B, long long lane)
{
    const long long nB = (long long)n_imu * B;
    // pass 1: omega, cf; the filter returns early when no IMU of the environment moves
    bool moving = false;
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        const T kp = (T)dt[s * ATT_IMU_DOUBLES];
        const V3<T> v = attitude_tilt(deform_load_quat(quat, s, nB, B, lane));
        const T * g = imu + (long long)s * 6 * B + lane;
        const T ax = g[3 * B] / T(9.81), ay = g[4 * B] / T(9.81), az = g[5 * B] / T(9.81);
        const T mx = ay * v.z - az * v.y, my = az * v.x - ax * v.z, mz = ax * v.y - ay * v.x;
        const T ox = g[0] - bias[o], oy = g[B] - bias[nB + o], oz = g[2 * B] - bias[2 * nB + o];
        omega[o] = ox; omega[nB + o] = oy; omega[2 * nB + o] = oz;
        const T cx = ox + kp * mx, cy = oy + kp * my, cz = oz + kp * mz;
        cf[o] = cx; cf[nB + o] = cy; cf[2 * nB + o] = cz;
        const T eps = T(1e-6);
        moving |= !((cx < T(0) ? -cx : cx) < eps && (cy < T(0) ? -cy : cy) < eps && (cz < T(0) ? -cz : cz) < eps);
    }
    // pass 2: integrate the orientation, update the bias estimate
    if (moving)
        for (int s = 0; s < n_imu; ++s)
        {
            const long long o = (long long)s * B + lane;
            const T ki = (T)dt[s * ATT_IMU_DOUBLES + 1];
            const T cx = cf[o], cy = cf[nB + o], cz = cf[2 * nB + o];
            const T theta = sqrt_(cx * cx + cy * cy + cz * cz);
            const T half = theta * (step / T(2));
            T sh, ch;
            sincos_(half, &sh, &ch);
            const T px = cx / theta * sh, py = cy / theta * sh, pz = cz / theta * sh, pw = ch;
            const Quat<T> p = deform_load_quat(quat, s, nB, B, lane);
            const Quat<T> n = {p.x * pw + p.w * px - p.z * py + p.y * pz, p.y * pw + p.z * px + p.w * py - p.x * pz,
                               p.z * pw - p.y * px + p.x * py + p.w * pz, p.w * pw - p.x * px - p.y * py - p.z * pz};
            attitude_store_quat(quat, nB, o, deform_renorm(n));
            const V3<T> v = attitude_tilt(p);
            const T * g = imu + (long long)s * 6 * B + lane;
            const T ax = g[3 * B] / T(9.81), ay = g[4 * B] / T(9.81), az = g[5 * B] / T(9.81);
            const T mx = ay * v.z - az * v.y, my = az * v.x - ax * v.z, mz = ax * v.y - ay * v.x;
            bias[o] -= ki * step * mx; bias[nB + o] -= ki * step * my; bias[2 * nB + o] -= ki * step * mz;
        }
    if (ignore_twist || rpy) attitude_swing_and_rpy<T>(n_imu, ignore_twist != 0, quat, rpy, B, lane);
}

// `BodyObserver.refresh_observation` (body_orientation_observer.py:237-266) for one lane.  imu_quat, quat `[4][n_imu][B]`;
// imu_omega, omega, rpy `[3][n_imu][B]`; twist `[n_imu][B]`.  twist_mode 0: keep the estimate; 1: remove the twist;
// 2: remove it and integrate it (`update_twist`, :58-71).
template<class T>
JM_DEV void body_observer_lane(const double * __restrict__ dt, int n_imu, const T * __restrict__ imu_quat,
                               const T * __restrict__ imu_omega, T * __restrict__ quat, T * __restrict__ omega,
                               T * __restrict__ twist, int twist_mode, double time_constant_inv, double step_, T * __restrict__ rpy,
                               long long B, long long lane)
{
    const long long nB = (long long)n_imu * B;
    bool singular = false;
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        const double * d = dt + s * ATT_IMU_DOUBLES + 2;
        const Quat<T> rel = {(T)d[0], (T)d[1], (T)d[2], (T)d[3]};
        const Quat<T> e = deform_qmul(deform_load_quat(imu_quat, s, nB, B, lane), rel, T(1), T(-1));
        if (twist_mode) singular |= attitude_tilt(e).z < T(-1) + T(1e-5);
        attitude_store_quat(quat, nB, o, e);
        // `quat_apply` (utils/math.py:687-705)
        const T xx = rel.x * rel.x, xy = rel.x * rel.y, xz = rel.x * rel.z, xw = rel.x * rel.w;
        const T yy = rel.y * rel.y, yz = rel.y * rel.z, yw = rel.y * rel.w, zz = rel.z * rel.z, zw = rel.z * rel.w, ww = rel.w * rel.w;
        const T x = imu_omega[o], y = imu_omega[nB + o], z = imu_omega[2 * nB + o];
        omega[o] = x * (xx + ww - yy - zz) + y * (T(2) * xy - T(2) * zw) + z * (T(2) * xz + T(2) * yw);
        omega[nB + o] = x * (T(2) * zw + T(2) * xy) + y * (ww - xx + yy - zz) + z * (-T(2) * xw + T(2) * yz);
        omega[2 * nB + o] = x * (-T(2) * yw + T(2) * xz) + y * (T(2) * xw + T(2) * yz) + z * (ww - xx - yy + zz);
    }
    if (twist_mode == 0)
    {
        if (rpy) attitude_swing_and_rpy<T>(n_imu, false, quat, rpy, B, lane);
        return;
    }
    // (the leak factor is a host float in the reference: `max(0.0, 1.0 - time_constant_inv * dt)`, :62)
    const T leak = twist_mode == 2 ? (T)fmax_(0.0, 1.0 - time_constant_inv * step_) : T(0), step = (T)step_;
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        Quat<T> e = deform_load_quat(quat, s, nB, B, lane);
        const V3<T> v = attitude_tilt(e);
        e = deform_swing(v.x, v.y, v.z, singular);
        if (twist_mode == 2)
        {
            const T dtwist = (-e.y * omega[o] + e.x * omega[nB + o]) / e.w + omega[2 * nB + o];
            T tw = twist[o] * leak;
            tw += dtwist * step;
            twist[o] = tw;
            T pz, pw;
            sincos_(T(0.5) * tw, &pz, &pw);
            e = {pw * e.x - pz * e.y, pz * e.x + pw * e.y, pz * e.w, pw * e.w};
        }
        attitude_store_quat(quat, nB, o, e);
        if (rpy) attitude_store_rpy(rpy, nB, o, e);
    }
}

#ifndef JM_HOST_EMU
struct AttitudeArgs
{
    const int32_t * it;
    const double * dt;
    int n_imu;
};
template<class T>
__global__ void __launch_bounds__(256) k_attitude_init(const AttitudeArgs p, int exact_init, const T * __restrict__ q,
                                                        const T * __restrict__ imu, const uint8_t * __restrict__ lane_mask,
                                                        T * __restrict__ quat, T * __restrict__ omega, T * __restrict__ cf,
                                                        T * __restrict__ bias, T * __restrict__ twist, T * __restrict__ rpy, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (lane_mask && !lane_mask[lane]) return;
    attitude_init_lane<T>(p.it, p.dt, p.n_imu, exact_init, q, imu, quat, omega, cf, bias, twist, rpy, B, lane);
}

template<class T>
__global__ void __launch_bounds__(256) k_mahony_observer(const AttitudeArgs p, const T * __restrict__ imu, T * __restrict__ quat,
                                                          T * __restrict__ omega, T * __restrict__ cf, T * __restrict__ bias,
                                                          double dt, int ignore_twist, T * __restrict__ rpy, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    mahony_observer_lane<T>(p.dt, p.n_imu, imu, quat, omega, cf, bias, (T)dt, ignore_twist, rpy, B, lane);
}

template<class T>
__global__ void __launch_bounds__(256) k_body_observer(const AttitudeArgs p, const T * __restrict__ imu_quat,
                                                        const T * __restrict__ imu_omega, T * __restrict__ quat,
                                                        T * __restrict__ omega, T * __restrict__ twist, int twist_mode,
                                                        double time_constant_inv, double dt, T * __restrict__ rpy, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    body_observer_lane<T>(p.dt, p.n_imu, imu_quat, imu_omega, quat, omega, twist, twist_mode, time_constant_inv, dt, rpy, B, lane);
}
#endif
}  // namespace jm
