// jm_attitude.h -- the attitude observers of gym_jiminy as batched HIP kernels: what the `MahonyFilter` class does around
// its numba function (per-IMU gains, twist removal, Euler angles, initialisation at the first refresh of an episode), that
// function on its own, and the `BodyObserver` block.  Every lane is one environment, arrays are `[rows][B]` like the physics
// state and the blocks of jm_blocks.h; the quaternion functions and the segment record are those of jm_rotation.h.
//
// Reference (numba / numpy code restated here per lane):
//   MahonyFilter.refresh_observation   python/gym_jiminy/common/gym_jiminy/common/blocks/mahony_filter.py:337-393
//   mahony_filter                      mahony_filter.py:28-101
//   BodyObserver.refresh_observation   python/gym_jiminy/common/gym_jiminy/common/blocks/body_orientation_observer.py:237-266
//   update_twist                       body_orientation_observer.py:26-71
//   remove_twist_from_quat             python/gym_jiminy/common/gym_jiminy/common/utils/math.py:1202-1244
//   quat_apply                         utils/math.py:645-709
// `swing_from_vector` on the IMUs of one environment decides its singular branch with `np.any` over them: the flag handed to
// it is "any IMU of the lane".  The three observer kernels take the tilt in its TILT_ROUNDED form, the plain function in its
// TILT_FUSED form (jm_rotation.h).
//
// The true IMU orientations of the exact initialisation (the reference reads `oMf` of pinocchio, :357-366) are a
// rotation-only walk from the root to the sensor frame over the lane's `q` rows: per IMU a list of segments (constant
// rotation, then a joint rotation read from `q`).  All lanes interpret the same tables: their reads are indexed by loop
// counters only and become scalar loads; per-lane state is one rotation matrix and one quaternion in registers.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "jm_rotation.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_imu, offset of the segment ints, n_imu x (first segment, segment count),
// segment ints]; `dt` (float64) = n_imu x (kp, ki, rel_quat xyzw), then the segments of jm_rotation.h (index = first row of
// `q`, no ratio).
constexpr int ATT_IMU_DOUBLES = 6;
constexpr int ATT_MAX_SEGS_PER_IMU = 256;

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
        if (kind < 0 || kind > SEG_QUAT)
        { why = "jm_attitude_plan_create: segment " + std::to_string(s) + " has an unknown joint kind"; return false; }
        const int rows = kind == SEG_NONE ? 0 : (kind == SEG_QUAT ? 4 : (kind == SEG_UNBOUNDED ? 2 : 1));
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
    dt.clear();
    for (int s = 0; s < d->n_imu; ++s)
    {
        dt.push_back(d->kp[s]);
        dt.push_back(d->ki[s]);
        dt.insert(dt.end(), d->rel_quat + 4 * s, d->rel_quat + 4 * s + 4);
    }
    pack_segments(d->n_seg, d->seg_kind, d->seg_q_index, d->seg_rot, d->seg_axis, nullptr, it, dt);
    return true;
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
            singular |= quat_tilt<TILT_ROUNDED>(quat_load(quat, s, nB, B, lane)).z < T(-1) + T(1e-5);
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        Quat<T> q = quat_load(quat, s, nB, B, lane);
        if (remove_twist)
        {
            const V3<T> v = quat_tilt<TILT_ROUNDED>(q);
            q = swing_from_vector(v.x, v.y, v.z, singular);
            quat_store(quat, nB, o, q);
        }
        if (rpy) quat_store_rpy(rpy, nB, o, q);
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
        const double * d = seg + (long long)s * SEG_DOUBLES;
        const M3<T> Cm = {(T)d[0], (T)d[1], (T)d[2], (T)d[3], (T)d[4], (T)d[5], (T)d[6], (T)d[7], (T)d[8]};
        R = s == s0 ? Cm : R * Cm;
        const int kind = it[si + 2 * s];
        if (kind == SEG_NONE) continue;
        const T * qr = q + (long long)it[si + 2 * s + 1] * B + lane;
        M3<T> J;
        if (kind == SEG_QUAT) J = quat_to_matrix<T>(qr[0], qr[B], qr[2 * B], qr[3 * B]);
        else if (kind == SEG_UNBOUNDED) J = rot_rodrigues<T>(v3((T)d[9], (T)d[10], (T)d[11]), qr[0], qr[B]);
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
        if (exact) e = matrix_to_quat(attitude_frame_rot<T>(it, dt, s, q, B, lane));
        else
        {
            const T * g = imu + (long long)s * 6 * B + lane;
            const T ax = g[3 * B], ay = g[4 * B], az = g[5 * B];
            const T n = sqrt_(ax * ax + ay * ay + az * az);
            e = swing_from_vector(ax / n, ay / n, az / n, singular);
        }
        quat_store(quat, nB, o, e);
        omega[o] = T(0); omega[nB + o] = T(0); omega[2 * nB + o] = T(0);
        cf[o] = T(0); cf[nB + o] = T(0); cf[2 * nB + o] = T(0);
        bias[o] = T(0); bias[nB + o] = T(0); bias[2 * nB + o] = T(0);
        if (twist) twist[o] = T(0);
        if (rpy) quat_store_rpy(rpy, nB, o, e);
    }
}

// where `mahony_filter` takes the gains of IMU s from: the two scalars of the plain function, or the plan
template<class T> struct UniformGains
{
    T kp_, ki_;
    JM_DEV T kp(int) const { return kp_; }
    JM_DEV T ki(int) const { return ki_; }
};
template<class T> struct PlanGains
{
    const double * dt;
    JM_DEV T kp(int s) const { return (T)dt[s * ATT_IMU_DOUBLES]; }
    JM_DEV T ki(int s) const { return (T)dt[s * ATT_IMU_DOUBLES + 1]; }
};

// `mahony_filter` (mahony_filter.py:28-101) for one lane, F the form of the tilt.  (No `__restrict__` here: `jm_block_mahony_filter`
// never promised it; the observer kernel's own parameters carry it.)  imu raw field `[n_imu][6][B]` (gyro 0-2, accel 3-5); quat `[4][n_imu][B]`; omega, cf, bias `[3][n_imu][B]`.
template<TiltForm F, class T, class Gains>
JM_DEV void mahony_lane(int n_imu, const Gains gains, const T * imu, T * quat, T * omega, T * cf, T * bias, T step, long long B,
                        long long lane)
{
    const long long nB = (long long)n_imu * B;
    // pass 1: omega, cf; the reference returns early when no IMU of the environment moves
    bool moving = false;
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        const T kp = gains.kp(s);
        const V3<T> v = quat_tilt<F>(quat_load(quat, s, nB, B, lane));
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
    if (!moving) return;
    // pass 2: integrate the orientation, update the bias estimate
    for (int s = 0; s < n_imu; ++s)
    {
        const long long o = (long long)s * B + lane;
        const T ki = gains.ki(s);
        const T cx = cf[o], cy = cf[nB + o], cz = cf[2 * nB + o];
        const T theta = sqrt_(cx * cx + cy * cy + cz * cz);
        const T half = theta * (step / T(2));
        T sh, ch;
        sincos_(half, &sh, &ch);
        const T px = cx / theta * sh, py = cy / theta * sh, pz = cz / theta * sh, pw = ch;
        const Quat<T> p = quat_load(quat, s, nB, B, lane);
        const Quat<T> n = {p.x * pw + p.w * px - p.z * py + p.y * pz, p.y * pw + p.z * px + p.w * py - p.x * pz,
                           p.z * pw - p.y * px + p.x * py + p.w * pz, p.w * pw - p.x * px - p.y * py - p.z * pz};
        quat_store(quat, nB, o, quat_renorm(n));
        const V3<T> v = quat_tilt<F>(p);
        const T * g = imu + (long long)s * 6 * B + lane;
        const T ax = g[3 * B] / T(9.81), ay = g[4 * B] / T(9.81), az = g[5 * B] / T(9.81);
        const T mx = ay * v.z - az * v.y, my = az * v.x - ax * v.z, mz = ax * v.y - ay * v.x;
        bias[o] -= ki * step * mx; bias[nB + o] -= ki * step * my; bias[2 * nB + o] -= ki * step * mz;
    }
}

// One tick of an initialised `MahonyFilter` (mahony_filter.py:376-393) for one lane: `mahony_filter` with the gains of
// every IMU, then the twist removal and the Euler angles -- which run after the filter's early return as well.
template<class T>
JM_DEV void mahony_observer_lane(const double * __restrict__ dt, int n_imu, const T * __restrict__ imu, T * __restrict__ quat,
                                 T * __restrict__ omega, T * __restrict__ cf, T * __restrict__ bias, T step, int ignore_twist,
                                 T * __restrict__ rpy, long long B, long long lane)
{
    mahony_lane<TILT_ROUNDED>(n_imu, PlanGains<T>{dt}, imu, quat, omega, cf, bias, step, B, lane);
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
        const Quat<T> e = quat_mul(quat_load(imu_quat, s, nB, B, lane), rel, T(1), T(-1));
        if (twist_mode) singular |= quat_tilt<TILT_ROUNDED>(e).z < T(-1) + T(1e-5);
        quat_store(quat, nB, o, e);
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
        Quat<T> e = quat_load(quat, s, nB, B, lane);
        const V3<T> v = quat_tilt<TILT_ROUNDED>(e);
        e = swing_from_vector(v.x, v.y, v.z, singular);
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
        quat_store(quat, nB, o, e);
        if (rpy) quat_store_rpy(rpy, nB, o, e);
    }
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_mahony(int n_imu, const T * imu, T * quat, T * omega, T * cf, T * bias,
                                                 double kp, double ki, double dt, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    mahony_lane<TILT_FUSED>(n_imu, UniformGains<T>{(T)kp, (T)ki}, imu, quat, omega, cf, bias, (T)dt, B, lane);
}

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
