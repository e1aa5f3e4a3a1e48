// jm_trajectory.h -- the reference side of the trajectory-tracking layer as one batched HIP kernel: the state of a recorded
// trajectory at each lane's own query time.  A device-resident dataset of named trajectories (built once, immutable
// afterwards, like the reference's `lock()`), a per-lane selection and time offset, and per launch one gather with the mode
// handling, the bisection, the Lie-group interpolation of `q`, the linear interpolation of the other fields and the odometry
// of the free-flyer when the time wraps.  Every lane is one environment, outputs are `[rows][B]` like the physics state.
//
// Reference (restated per lane, operation for operation):
//   Trajectory.get                    python/jiminy_py/src/jiminy_py/dynamics.py:296-388 (TRAJ_INTERP_TOL :31)
//   Trajectory.__init__ (stride)      dynamics.py:207-213 -- computed once on the host (jiminy_amd/trajectory.py), float64
//   DatasetTrajectoryQuantity         python/gym_jiminy/common/gym_jiminy/common/bases/quantities.py:870-1210
//   log6 / log3, exp6 / exp3          gym_jiminy/common/utils/math.py:842-894 / 725-774, 908-954 / 791-825, written the way
//                                     `frame_average_lane` of jm_frames.h states them (its rounded quaternion product: two equal
//                                     samples interpolate to exactly that sample)
//   BaseOdometryPose                  gym_jiminy/common/quantities/locomotion.py:158-220, the expression of jm_locomotion.h
// `pin.interpolate` is `integrate(q0, alpha * difference(q0, q1))` joint by joint: a vector-space joint q0 + alpha (q1 - q0),
// the free-flyer M0 exp6(alpha log6(M0^-1 M1)), a spherical joint quat0 exp3(alpha log3(quat0^-1 quat1)), an unbounded
// revolute joint the same on its angle.  The wrap odometry is `exp6(n_steps * stride) * M(q[:7])`: the translation with `exp6`
// of jm_math.h (a stride of zero takes its Taylor branch and is the identity), the rotation as the quaternion of `exp3`.
//
// The query time, the mode handling, the search and `alpha` are float64 whatever the batch's dtype: a tolerance of 1e-10
// means nothing in float32.  The device cannot raise: mode `raise` sets bit 0 of the lane's flags and goes on with the
// clipped time; a lane whose trajectory index is outside the dataset sets bit 1 and writes nothing else.  The search keeps no
// per-lane state: for non-decreasing times the reference's cached index only shortens it.
//
// The samples are sample-major, `data [S][R]` in the batch's dtype, a row the present fields concatenated: q (nq), then v (nv),
// a (nv), command (n_command) where present.  The left and the right sample of a lane are adjacent rows: one contiguous span.
// The joint table and the motor rows are read through loop counters only and become scalar loads; what depends on the
// lane's trajectory (mode, sample range, stride, times) is a per-lane load.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "jm_frames.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [N, S, nq, nv, n_command, fields, R, n_joints, n_motors, has_freeflyer,
// n_joints x (kind, first q row), n_motors x q row, N x mode, (N + 1) x sample_start]; `dt` (float64) = [N x 6 stride, S times].
constexpr int TRAJ_HEAD_INTS = 10;
constexpr int TRAJ_RAISE = 0, TRAJ_WRAP = 1, TRAJ_CLIP = 2;
constexpr int TRAJ_HAS_V = 1, TRAJ_HAS_A = 2, TRAJ_HAS_COMMAND = 4;
constexpr int TRAJ_FLAG_OUT_OF_RANGE = 1, TRAJ_FLAG_BAD_TRAJECTORY = 2;
constexpr int TRAJ_STATUS_FLAGS = 0, TRAJ_STATUS_N_STEPS = 1, TRAJ_STATUS_INDEX = 2;
constexpr double TRAJ_INTERP_TOL = 1e-10;     // dynamics.py:31

inline int trajectory_row_size(int nq, int nv, int n_command, int fields)
{
    return nq + ((fields & TRAJ_HAS_V) ? nv : 0) + ((fields & TRAJ_HAS_A) ? nv : 0) + ((fields & TRAJ_HAS_COMMAND) ? n_command : 0);
}

// Validate a description and pack its tables (the samples are uploaded apart).  Returns false and a message on a malformed
// description.
inline bool trajectory_pack(const jm_trajectory_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_trajectory_plan_create: ";
    if (!d) { why = who + "null description"; return false; }
    if (d->dtype != JM_F64 && d->dtype != JM_F32) { why = who + "bad dtype"; return false; }
    if (!d->sample_start || !d->times || !d->mode || !d->data || !d->joint_kind || !d->joint_q_index)
    { why = who + "null array in the description"; return false; }
    if (d->n_trajectories <= 0 || d->n_samples <= 0 || d->nq <= 0 || d->nv < 0 || d->n_command < 0 || d->n_joints <= 0 || d->n_motors < 0)
    { why = who + "bad sizes"; return false; }
    if (d->fields < 0 || d->fields > (TRAJ_HAS_V | TRAJ_HAS_A | TRAJ_HAS_COMMAND))
    { why = who + "unknown field bits (1: v, 2: a, 4: command)"; return false; }
    if (((d->fields & (TRAJ_HAS_V | TRAJ_HAS_A)) && d->nv <= 0) || ((d->fields & TRAJ_HAS_COMMAND) && d->n_command <= 0))
    { why = who + "a present field has no rows"; return false; }
    if (d->n_motors > 0 && !d->motor_q_index) { why = who + "null array in the description"; return false; }
    const int N = d->n_trajectories, S = d->n_samples;
    if (d->sample_start[0] != 0 || d->sample_start[N] != S) { why = who + "sample_start must run from 0 to n_samples"; return false; }
    bool freeflyer = false;
    for (int j = 0; j < d->n_joints; ++j)
    {
        const int kind = d->joint_kind[j], qi = d->joint_q_index[j];
        const std::string joint = "joint " + std::to_string(j);
        if (kind <= SEG_NONE || kind > FR_PAXIS) { why = who + joint + " has an unknown joint kind"; return false; }
        const int n = frames_nq_of(kind);
        if (qi < 0 || qi + n > d->nq)
        { why = who + joint + " reads q rows [" + std::to_string(qi) + ", " + std::to_string(qi + n) + ") out of range [0, " +
                std::to_string(d->nq) + ")"; return false; }
        if (kind == FR_FREEFLYER)
        {
            // (the reference's odometry is `position[:7]`, and a model has one root)
            if (j != 0 || qi != 0) { why = who + joint + ": a free-flyer must be joint 0 at q row 0"; return false; }
            freeflyer = true;
        }
    }
    if (freeflyer && !d->stride) { why = who + "a free-flyer needs the strides"; return false; }
    for (int m = 0; m < d->n_motors; ++m)
    {
        const int row = d->motor_q_index[m];
        bool found = false;
        for (int j = 0; j < d->n_joints; ++j) found |= d->joint_q_index[j] == row && frames_nq_of(d->joint_kind[j]) == 1;
        if (row < 0 || row >= d->nq || !found)
        { why = who + "motor " + std::to_string(m) + " reads q row " + std::to_string(row) + ", which is not the row of a one-row joint";
          return false; }
    }
    for (int k = 0; k < N; ++k)
    {
        const std::string traj = "trajectory " + std::to_string(k);
        const int s0 = d->sample_start[k], s1 = d->sample_start[k + 1];
        if (s0 < 0 || s1 > S || s1 - s0 < 2) { why = who + traj + " needs at least 2 samples inside the dataset"; return false; }
        for (int s = s0; s < s1; ++s)
        {
            if (!std::isfinite(d->times[s])) { why = who + traj + " has a time that is not finite (sample " + std::to_string(s - s0) + ")"; return false; }
            if (s > s0 && d->times[s] - d->times[s - 1] < 0.0)
            { why = who + traj + ": time must not be decreasing between consecutive timesteps (sample " + std::to_string(s - s0) + ")"; return false; }
        }
        if (d->mode[k] < TRAJ_RAISE || d->mode[k] > TRAJ_CLIP) { why = who + traj + " has an unknown time mode (0 raise, 1 wrap, 2 clip)"; return false; }
        if (freeflyer)
            for (int c = 0; c < 6; ++c)
                if (!std::isfinite(d->stride[6 * k + c])) { why = who + traj + " has a stride that is not finite"; return false; }
    }
    it = {N, S, d->nq, d->nv, d->n_command, d->fields, trajectory_row_size(d->nq, d->nv, d->n_command, d->fields), d->n_joints,
          d->n_motors, freeflyer ? 1 : 0};
    for (int j = 0; j < d->n_joints; ++j) { it.push_back(d->joint_kind[j]); it.push_back(d->joint_q_index[j]); }
    for (int m = 0; m < d->n_motors; ++m) it.push_back(d->motor_q_index[m]);
    it.insert(it.end(), d->mode, d->mode + N);
    it.insert(it.end(), d->sample_start, d->sample_start + N + 1);
    dt.clear();
    for (int k = 0; k < 6 * N; ++k) dt.push_back(freeflyer ? d->stride[k] : 0.0);
    dt.insert(dt.end(), d->times, d->times + S);
    return true;
}

// the inputs and the outputs of one launch (device pointers); every output may be null
template<class T> struct TrajIO
{
    const double * time;            // [B] episode time of the lane
    const int32_t * trajectory;     // [B]
    const double * time_offset;     // [B]
    const uint8_t * lane_mask;      // [B]
    T * q;                          // [nq][B]
    T * v; T * a;                   // [nv][B]
    T * command;                    // [n_command][B]
    T * odom_pose;                  // [3][B] x, y, yaw of the free-flyer
    T * position;                   // [n_motors][B] q[idx_q]
    int32_t * status;               // [3][B] flags, n_steps, right index
};

// `log3` (utils/math.py:766-770) of a unit quaternion; `sin_2` and `theta` are what `log6` goes on with
template<class T> JM_DEV V3<T> traj_log3(const Quat<T> & qd, T & sin_2, T & theta)
{
    sin_2 = sqrt_(qd.x * qd.x + qd.y * qd.y + qd.z * qd.z);
    theta = T(2) * atan2_(sin_2, fabs_(qd.w));
    const T inv_sinc = theta / fmax_(sin_2, FrameTiny<T>::tiny), sg = frame_sign(qd.w);
    return v3(inv_sinc * qd.x * sg, inv_sinc * qd.y * sg, inv_sinc * qd.z * sg);
}

// `log6` (utils/math.py:876-890) of the pose (pos, qd)
template<class T> JM_DEV Sp<T> traj_log6(V3<T> pos, const Quat<T> & qd)
{
    T sin_2, theta;
    const V3<T> ang = traj_log3(qd, sin_2, theta);
    const T eps = FrameTiny<T>::root;
    const T cot_2 = fabs_(qd.w) / fmax_(sin_2, eps);
    theta = fmax_(theta, eps);
    const T beta = T(1) / (theta * theta) - T(0.5) * cot_2 / theta;
    const V3<T> wxv = cross(ang, pos), w2xv = cross(ang, wxv);
    return {v3(pos.x - T(0.5) * wxv.x + beta * w2xv.x, pos.y - T(0.5) * wxv.y + beta * w2xv.y, pos.z - T(0.5) * wxv.z + beta * w2xv.z),
            ang};
}

// `exp3` (utils/math.py:815-821)
template<class T> JM_DEV Quat<T> traj_exp3(V3<T> va)
{
    const T th = sqrt_(va.x * va.x + va.y * va.y + va.z * va.z), den = fmax_(th, FrameTiny<T>::tiny);
    T sh, ch;
    sincos_(T(0.5) * th, &sh, &ch);
    return {sh * (va.x / den), sh * (va.y / den), sh * (va.z / den), ch};
}

// `exp6` (utils/math.py:929-950): the translation; the rotation is `traj_exp3` of the angular part
template<class T> JM_DEV V3<T> traj_exp6_translation(const Sp<T> & nu)
{
    const V3<T> vl = nu.l, va = nu.a;
    const T sum_sq = va.x * va.x + va.y * va.y + va.z * va.z;
    const T theta_sq = fmax_(sum_sq, FrameTiny<T>::pow23), th = sqrt_(theta_sq);
    T sn, cs;
    sincos_(th, &sn, &cs);
    const T alpha_wxv = (T(1) - cs) / theta_sq, alpha_w2 = (th - sn) / theta_sq / th;
    const V3<T> wxv = cross(va, vl), w2xv = cross(va, wxv);
    return v3(vl.x + alpha_wxv * wxv.x + alpha_w2 * w2xv.x, vl.y + alpha_wxv * wxv.y + alpha_w2 * w2xv.y,
              vl.z + alpha_wxv * wxv.z + alpha_w2 * w2xv.z);
}

// left + alpha (right - left): every field but `q`, and the vector-space joints of `q`
template<class T> JM_DEV T traj_lerp(T left, T right, T alpha) { return left + alpha * (right - left); }

// one row of a vector space: the copy of a sample (`pick` 0 left, 1 right) or the interpolation
template<class T> JM_DEV T traj_row(const T * __restrict__ left, const T * __restrict__ right, int row, int pick, T alpha)
{
    return pick == 0 ? left[row] : pick == 1 ? right[row] : traj_lerp(left[row], right[row], alpha);
}

// a block of rows of a vector space into `out [rows][B]`
template<class T>
JM_DEV void traj_rows(T * __restrict__ out, const T * __restrict__ left, const T * __restrict__ right, int first, int rows, int pick,
                      T alpha, long long B, long long lane)
{
    if (!out) return;
    for (int r = 0; r < rows; ++r) out[(long long)r * B + lane] = traj_row(left, right, first + r, pick, alpha);
}

// The state of the lane's trajectory at the lane's time.
template<class T>
JM_DEV void trajectory_state_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, const T * __restrict__ data,
                                  const TrajIO<T> & io, long long B, long long lane)
{
    const int N = it[0], nq = it[2], nv = it[3], n_cmd = it[4], fields = it[5], R = it[6], n_joints = it[7], M = it[8];
    const bool freeflyer = it[9] != 0;
    const int32_t * joints = it + TRAJ_HEAD_INTS;
    const int32_t * motors = joints + 2 * n_joints;
    const int32_t * modes = motors + M;
    const int32_t * sample_start = modes + N;
    const double * times = dt + 6 * (long long)N;

    const int traj = io.trajectory[lane];
    if (traj < 0 || traj >= N)
    {
        if (io.status)
        {
            io.status[(long long)TRAJ_STATUS_FLAGS * B + lane] = TRAJ_FLAG_BAD_TRAJECTORY;
            io.status[(long long)TRAJ_STATUS_N_STEPS * B + lane] = 0;
            io.status[(long long)TRAJ_STATUS_INDEX * B + lane] = 0;
        }
        return;
    }
    const int s0 = sample_start[traj], n = sample_start[traj + 1] - s0, mode = modes[traj];
    const double * tm = times + s0;
    const double t_start = tm[0], t_end = tm[n - 1];

    // ---- the mode (dynamics.py:326-336)
    double t = io.time[lane] + io.time_offset[lane];
    int flags = 0, n_steps = 0;
    if (!(t - t == 0.0))
    {
        // (a time that is not finite has no place in any mode)
        flags = TRAJ_FLAG_OUT_OF_RANGE;
        t = t_start;
    }
    else if (mode == TRAJ_WRAP)
    {
        if (t_end > t_start)
        {
            // Python's `divmod` of two floats: the exact remainder, moved by one span where its sign differs from the span's,
            // and the matching floored quotient
            const double x = t - t_start, span = t_end - t_start;
            double mod = ::fmod(x, span);
            double div = (x - mod) / span;
            if (mod != 0.0)
            {
                if (mod < 0.0) { mod += span; div -= 1.0; }
            }
            else mod = 0.0;
            double steps = 0.0;
            if (div != 0.0)
            {
                steps = ::floor(div);
                if (div - steps > 0.5) steps += 1.0;
            }
            n_steps = (int)::fmin(::fmax(steps, -2147483647.0), 2147483647.0);
            t = mod + t_start;
        }
        else t = t_start;
    }
    else
    {
        if (mode == TRAJ_RAISE && (t - t_end > TRAJ_INTERP_TOL || t_start - t > TRAJ_INTERP_TOL)) flags = TRAJ_FLAG_OUT_OF_RANGE;
        t = ::fmin(::fmax(t, t_start), t_end);
    }

    // ---- `bisect_left(times, t, 1, n - 1)` (dynamics.py:347-348)
    int lo = 1, hi = n - 1;
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (tm[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    const int index = lo;
    if (io.status)
    {
        io.status[(long long)TRAJ_STATUS_FLAGS * B + lane] = flags;
        io.status[(long long)TRAJ_STATUS_N_STEPS * B + lane] = n_steps;
        io.status[(long long)TRAJ_STATUS_INDEX * B + lane] = index;
    }

    // ---- the samples and the ratio (dynamics.py:352-359)
    const double t_left = tm[index - 1], t_right = tm[index];
    const int pick = t - t_left < TRAJ_INTERP_TOL ? 0 : t_right - t < TRAJ_INTERP_TOL ? 1 : 2;
    const T alpha = pick == 2 ? (T)((t - t_left) / (t_right - t_left)) : T(0);
    const T * left = data + (long long)(s0 + index - 1) * R;
    const T * right = left + R;

    // ---- q (dynamics.py:362-368), the free-flyer first and on its own
    if (freeflyer && (io.q || io.odom_pose))
    {
        V3<T> x;
        Quat<T> e;
        if (pick == 2)
        {
            const V3<T> x0 = v3(left[0], left[1], left[2]), x1 = v3(right[0], right[1], right[2]);
            const Quat<T> q0 = {left[3], left[4], left[5], left[6]}, q1 = {right[3], right[4], right[5], right[6]};
            Sp<T> nu = traj_log6(frame_quat_apply(q0, x1 - x0, T(-1)), frame_quat_mul(q0, q1, T(-1), T(1)));
            nu.l = alpha * nu.l; nu.a = alpha * nu.a;
            x = x0 + frame_quat_apply(q0, traj_exp6_translation(nu), T(1));
            e = frame_quat_mul(q0, traj_exp3(nu.a), T(1), T(1));
        }
        else
        {
            const T * s = pick == 0 ? left : right;
            x = v3(s[0], s[1], s[2]);
            e = {s[3], s[4], s[5], s[6]};
        }
        // the odometry of a wrapping time (dynamics.py:382-385), composed on the left
        if (n_steps != 0)
        {
            const double * st = dt + 6 * (long long)traj;
            const double k = (double)n_steps;
            const Sp<T> nu = {v3((T)(k * st[0]), (T)(k * st[1]), (T)(k * st[2])), v3((T)(k * st[3]), (T)(k * st[4]), (T)(k * st[5]))};
            // (the translation of `exp6` of jm_math.h, with its Taylor branch; the rotation as the quaternion of `exp3`, whose
            // sign follows the angle continuously, which the quaternion of a rotation matrix does not)
            const Quat<T> qs = traj_exp3(nu.a);
            x = exp6(nu).p + frame_quat_apply(qs, x, T(1));
            e = frame_quat_mul(qs, e, T(1), T(1));
        }
        if (io.q)
        {
            io.q[lane] = x.x; io.q[B + lane] = x.y; io.q[2 * B + lane] = x.z;
            io.q[3 * B + lane] = e.x; io.q[4 * B + lane] = e.y; io.q[5 * B + lane] = e.z; io.q[6 * B + lane] = e.w;
        }
        if (io.odom_pose)
        {
            // `BaseOdometryPose` (quantities/locomotion.py:211-219), the expression of `locomotion_lane`
            const T qx = e.x, qy = e.y, qz = e.z, qw = e.w;
            const T q_xy = qy * qx, q_yy = qy * qy, q_zz = qz * qz, q_zw = qz * qw;    // (utils/math.py:103-105)
            const T yaw = atan2_(T(2) * (q_xy + q_zw), T(1) - T(2) * (q_yy + q_zz));
            io.odom_pose[lane] = x.x; io.odom_pose[B + lane] = x.y; io.odom_pose[2 * B + lane] = yaw;
        }
    }
    if (io.q)
        for (int j = freeflyer ? 1 : 0; j < n_joints; ++j)
        {
            const int kind = joints[2 * j], row = joints[2 * j + 1];
            T * out = io.q + (long long)row * B + lane;
            if (kind == SEG_QUAT)
            {
                Quat<T> e;
                if (pick == 2)
                {
                    const Quat<T> q0 = {left[row], left[row + 1], left[row + 2], left[row + 3]};
                    const Quat<T> q1 = {right[row], right[row + 1], right[row + 2], right[row + 3]};
                    T sin_2, theta;
                    const V3<T> w = traj_log3(frame_quat_mul(q0, q1, T(-1), T(1)), sin_2, theta);
                    e = frame_quat_mul(q0, traj_exp3(alpha * w), T(1), T(1));
                }
                else
                {
                    const T * s = (pick == 0 ? left : right) + row;
                    e = {s[0], s[1], s[2], s[3]};
                }
                out[0] = e.x; out[B] = e.y; out[2 * B] = e.z; out[3 * B] = e.w;
            }
            else if (kind == SEG_UNBOUNDED)
            {
                T c = (pick == 1 ? right : left)[row], s = (pick == 1 ? right : left)[row + 1];
                if (pick == 2)
                {
                    // the angle from the left to the right sample, then the left one turned by its share
                    const T c0 = left[row], s0_ = left[row + 1], c1 = right[row], s1 = right[row + 1];
                    const T angle = alpha * atan2_(frame_product(c0 * s1) - frame_product(s0_ * c1),
                                                   frame_product(c0 * c1) + frame_product(s0_ * s1));
                    T sa, ca;
                    sincos_(angle, &sa, &ca);
                    c = c0 * ca - s0_ * sa;
                    s = s0_ * ca + c0 * sa;
                }
                out[0] = c; out[B] = s;
            }
            else out[0] = traj_row(left, right, row, pick, alpha);
        }

    // ---- every other field (dynamics.py:370-379)
    int first = nq;
    if (fields & TRAJ_HAS_V) { traj_rows(io.v, left, right, first, nv, pick, alpha, B, lane); first += nv; }
    if (fields & TRAJ_HAS_A) { traj_rows(io.a, left, right, first, nv, pick, alpha, B, lane); first += nv; }
    if (fields & TRAJ_HAS_COMMAND) traj_rows(io.command, left, right, first, n_cmd, pick, alpha, B, lane);

    // ---- the joint-side motor positions `q[idx_q]`: rows of one-row joints, the expression of `q` itself
    if (io.position)
        for (int m = 0; m < M; ++m) io.position[(long long)m * B + lane] = traj_row(left, right, motors[m], pick, alpha);
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_trajectory_state(const int32_t * __restrict__ it, const double * __restrict__ dt,
                                                           const T * __restrict__ data, const TrajIO<T> io, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    trajectory_state_lane<T>(it, dt, data, io, B, lane);
}
#endif
}  // namespace jm
