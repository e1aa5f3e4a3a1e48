// jm_trackrewards.h -- the tracking rewards of the reference's composition layer on balance quantities as one batched HIP
// kernel: a quantity evaluated on the true state and on the state of the reference trajectory, and the radial basis function
// of their difference.  Every lane is one environment, arrays are `[rows][B]` like the physics state.  Everything is read
// from tensors other blocks left on the device: the two frame kinematics blocks (jm_frames.h), the two locomotion blocks
// (jm_locomotion.h), the actuated-joint block and the reference trajectory.
//
// Reference (python/gym_jiminy/common/gym_jiminy/common):
//   TrackingQuantityReward                 compositions/generic.py:64-122   rbf(true - reference, cutoff, 2)
//   TrackingBaseHeightReward               compositions/locomotion.py:33-51     `compute_height`, quantities/locomotion.py:88-97, :153
//   TrackingBaseOdometryVelocityReward     compositions/locomotion.py:54-72     quantities/locomotion.py:281-288 masked as in :329-333
//   TrackingCapturePointReward             compositions/locomotion.py:123-143   the `dcm` of jm_locomotion.h, LOCAL
//   TrackingActuatedJointPositionsReward   compositions/generic.py:125-150
//   radial_basis_function                  compositions/mixin.py:26-66          `loco_rbf` of jm_locomotion.h
#pragma once
#include "jm_locomotion.h"

namespace jm
{
// rows of `rewards`; `value` / `reference` hold the terms concatenated: height (1), odometry velocity (3), capture point (2),
// joint positions (n_motors)
constexpr int TR_HEIGHT = 0, TR_ODOM_VELOCITY = 1, TR_CAPTURE_POINT = 2, TR_JOINT_POSITIONS = 3, TR_TERMS = 4;
constexpr int TR_FIXED_ROWS = 6;
// ---- the packed plan: `it` = [n_contacts, n_motors, K, root column, K_reference, root column of the reference,
// n_contacts x column, n_contacts x column of the reference]; `dt` is empty but for one unused entry.
constexpr int TR_HEAD_INTS = 6;
constexpr int TR_MAX_CONTACTS = 64, TR_MAX_MOTORS = 256;

inline bool trackrewards_pack(const jm_trackrewards_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_trackrewards_plan_create: ";
    if (!d) { why = who + "null description"; return false; }
    if (d->n_contacts < 0 || d->n_contacts > TR_MAX_CONTACTS || d->n_motors < 0 || d->n_motors > TR_MAX_MOTORS || d->n_frames < 0 ||
        d->n_frames_reference < 0)
    { why = who + "bad sizes"; return false; }
    if (d->n_contacts > 0 && (!d->contact_column || !d->contact_column_reference))
    { why = who + "null array in the description"; return false; }
    const int32_t K[2] = {d->n_frames, d->n_frames_reference}, root[2] = {d->root_column, d->root_column_reference};
    const int32_t * col[2] = {d->contact_column, d->contact_column_reference};
    const char * side[2] = {"", " of the reference"};
    for (int s = 0; s < 2; ++s)
    {
        if (K[s] == 0) continue;    // (no frames block on this side: the terms that read one are skipped)
        if (root[s] < 0 || root[s] >= K[s])
        { why = who + "the root column" + side[s] + " is out of range [0, " + std::to_string(K[s]) + ")"; return false; }
        for (int c = 0; c < d->n_contacts; ++c)
            if (col[s][c] < 0 || col[s][c] >= K[s])
            { why = who + "contact " + std::to_string(c) + " has a column" + side[s] + " out of range [0, " + std::to_string(K[s]) + ")";
              return false; }
    }
    it = {d->n_contacts, d->n_motors, K[0], root[0], K[1], root[1]};
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < d->n_contacts; ++c) it.push_back(K[s] ? col[s][c] : 0);
    dt.assign(1, 0.0);
    return true;
}

template<class T> struct TrkRewIO
{
    const T * pose;                     // [7][K][B] of the true frames block
    const T * pose_reference;           // [7][K_ref][B]
    const T * v_avg;                    // [6][K][B] step-average velocity (root column: LOCAL)
    const T * quat_no_yaw;              // [4][K][B]
    const T * v_avg_reference;          // [6][K_ref][B]
    const T * quat_no_yaw_reference;    // [4][K_ref][B]
    const T * dcm;                      // [2][B] of the true locomotion block (LOCAL)
    const T * dcm_reference;            // [2][B]
    const T * position;                 // [M][B] of the actuated-joint block
    const T * position_reference;       // [M][B] of the reference trajectory
    const uint8_t * lane_mask;          // [B]
    T * value;                          // [6 + M][B]
    T * reference;                      // [6 + M][B]
    T * rewards;                        // [4][B]
};

// `compute_height` (quantities/locomotion.py:88-97): the root's z minus the lowest contact frame's
template<class T> JM_DEV T trackrewards_height(const T * __restrict__ pose, const int32_t * __restrict__ col, int nc, int root, long long KB,
                                               long long B, long long lane)
{
    const T * z = pose + 2 * KB + lane;
    T lowest = z[(long long)col[0] * B];
    // (the minimum propagates NaN like `np.min`; `fmin_` would drop it)
    for (int c = 1; c < nc; ++c)
    {
        const T x = z[(long long)col[c] * B];
        lowest = (x < lowest || x != x) ? x : lowest;
    }
    return z[(long long)root * B] - lowest;
}

// rows (0, 1, 5) of `quat_apply(quat_no_yaw, v_avg)` of the root column (quantities/locomotion.py:281-288, :329-333)
template<class T> JM_DEV V3<T> trackrewards_odom_velocity(const T * __restrict__ v_avg, const T * __restrict__ qny, int root, long long KB,
                                                          long long B, long long lane)
{
    const long long o = (long long)root * B + lane;
    const Quat<T> q = quat_load(qny, root, KB, B, lane);
    const V3<T> l = frame_quat_apply(q, v3(v_avg[o], v_avg[KB + o], v_avg[2 * KB + o]), T(1));
    const V3<T> g = frame_quat_apply(q, v3(v_avg[3 * KB + o], v_avg[4 * KB + o], v_avg[5 * KB + o]), T(1));
    return v3(l.x, l.y, g.z);
}

// All terms of one lane.  cutoff `[4]`: a term whose cutoff is not positive or whose inputs are null is skipped, its rows are
// left alone.  Every output may be null.
template<class T>
JM_DEV void trackrewards_lane(const int32_t * __restrict__ it, const TrkRewIO<T> & io, const double * __restrict__ cutoff, long long B,
                              long long lane)
{
    const int nc = it[0], M = it[1], K = it[2], root = it[3], Kr = it[4], root_r = it[5];
    const int32_t * col = it + TR_HEAD_INTS, * col_r = col + nc;
    const auto put = [&](int row, T value, T reference) {
        if (io.value) io.value[(long long)row * B + lane] = value;
        if (io.reference) io.reference[(long long)row * B + lane] = reference;
    };
    const auto reward = [&](int term, T sq_norm) {
        if (io.rewards) io.rewards[(long long)term * B + lane] = loco_rbf(sq_norm, (T)cutoff[term]);
    };
    if (cutoff[TR_HEIGHT] > 0.0 && io.pose && io.pose_reference && nc > 0 && K > 0 && Kr > 0)
    {
        const T h = trackrewards_height(io.pose, col, nc, root, (long long)K * B, B, lane);
        const T hr = trackrewards_height(io.pose_reference, col_r, nc, root_r, (long long)Kr * B, B, lane);
        put(0, h, hr);
        const T e = h - hr;
        reward(TR_HEIGHT, e * e);
    }
    if (cutoff[TR_ODOM_VELOCITY] > 0.0 && io.v_avg && io.quat_no_yaw && io.v_avg_reference && io.quat_no_yaw_reference && K > 0 && Kr > 0)
    {
        const V3<T> u = trackrewards_odom_velocity(io.v_avg, io.quat_no_yaw, root, (long long)K * B, B, lane);
        const V3<T> ur = trackrewards_odom_velocity(io.v_avg_reference, io.quat_no_yaw_reference, root_r, (long long)Kr * B, B, lane);
        put(1, u.x, ur.x); put(2, u.y, ur.y); put(3, u.z, ur.z);
        const V3<T> e = u - ur;
        reward(TR_ODOM_VELOCITY, e.x * e.x + e.y * e.y + e.z * e.z);
    }
    if (cutoff[TR_CAPTURE_POINT] > 0.0 && io.dcm && io.dcm_reference)
    {
        const T x = io.dcm[lane], y = io.dcm[B + lane], xr = io.dcm_reference[lane], yr = io.dcm_reference[B + lane];
        put(4, x, xr); put(5, y, yr);
        reward(TR_CAPTURE_POINT, (x - xr) * (x - xr) + (y - yr) * (y - yr));
    }
    if (cutoff[TR_JOINT_POSITIONS] > 0.0 && io.position && io.position_reference && M > 0)
    {
        T sq = T(0);
        for (int m = 0; m < M; ++m)
        {
            const T p = io.position[(long long)m * B + lane], pr = io.position_reference[(long long)m * B + lane];
            put(TR_FIXED_ROWS + m, p, pr);
            sq += (p - pr) * (p - pr);
        }
        reward(TR_JOINT_POSITIONS, sq);
    }
}

#ifndef JM_HOST_EMU
struct TrkRewCutoffs
{
    double c[TR_TERMS];
};
template<class T>
__global__ void __launch_bounds__(256) k_tracking_rewards(const int32_t * __restrict__ it, const TrkRewIO<T> io, const TrkRewCutoffs cutoff,
                                                           long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    trackrewards_lane<T>(it, io, cutoff.c, B, lane);
}
#endif
}  // namespace jm
