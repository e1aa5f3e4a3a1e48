// jm_tracking.h -- the trajectory-tracking windows of the reference's composition layer as one batched HIP kernel: the drift of
// the base odometry pose against a reference over a sliding window of environment steps (position and orientation, with the
// reward on the pair), and the shift of the relative foot poses and of the motor positions against their references: the
// smallest time-aligned distance inside a window.  Every lane is one environment, arrays are `[rows][B]` like the physics
// state.  Everything is read from what the other quantity blocks left in device memory: `odom_pose` of the locomotion
// quantities, `relative_pose` of the foot pose quantities, `position` of the actuated-joint quantities, and the reference
// tensors the caller fills.
//
// Reference (python/gym_jiminy/common/gym_jiminy/common, restated per lane, operation for operation):
//   StackedQuantity.refresh                       quantities/transform.py:208-296, both branches
//   DeltaQuantity                                 quantities/transform.py:715-831
//   DeltaBaseOdometryPosition                     quantities/locomotion.py:1537-1599 (bounds_only=True, op=sub)
//   angle_difference, DeltaBaseOdometryOrientation  quantities/locomotion.py:1602-1693 (bounds_only=False)
//   compute_drift_error,
//   DriftTrackingQuantityTermination              compositions/generic.py:194-315
//   DriftTrackingBaseOdometry{Position,Orientation}Termination  compositions/locomotion.py:623-736
//   min_norm, compute_min_distance,
//   ShiftTrackingQuantityTermination              compositions/generic.py:318-453
//   ShiftTrackingMotorPositionsTermination        compositions/generic.py:664-716
//   ShiftTrackingFootOdometryPositionsTermination compositions/locomotion.py:739-791
//   angle_distance,
//   ShiftTrackingFootOdometryOrientationsTermination  compositions/locomotion.py:794-867, with `quat_to_yaw` (utils/math.py:95-141)
//   l2_norm, DriftTrackingBaseOdometryPoseReward  compositions/locomotion.py:76-120: radial_basis_function(error, cutoff, 2)
//                                                 (compositions/mixin.py:17-66; `loco_rbf` of jm_locomotion.h)
//
// This generalises the power window of jm_actuation.h.  Three families, each optional and each with a window of its own
// (`max_stack = max(ceil(horizon / step_dt), 1) + 1`, 0: the family is absent), share one counter per lane, `count [B]`: the
// `num_steps` of the reference's stacks.  A launch has two modes: TRK_RESTART (count = 0) and TRK_PUSH (count += 1).  The
// state lives in arrays the caller owns:
//   odometry   `odom_ring [max_stack][4][B]` (true x, true y, reference x, reference y): the non-wrapping stack of
//              `DeltaQuantity(bounds_only=True)` kept as a ring: the newest value is the one of this launch, the oldest sits in
//              slot (count + 1) % max_stack once count + 1 >= max_stack and in slot 0 before: one per-lane address, no loop.
//              `yaw_prev [2][B]` and `yaw_ring [max_stack - 1][2][B]` (true, reference): the inner two-value stack and the
//              wrapping array of `DeltaQuantity(bounds_only=False)`: `angle_difference(yaw, yaw_prev)` goes into slot
//              count % (max_stack - 1) (at a restart the inner stack holds one value and gives op(v0, v0)), the delta is the sum
//              of the first min(count + 1, max_stack - 1) slots in storage order.
//   feet       `foot_ring [2][max_stack][B]`: per timestamp one squared norm per termination, not the values -- `min_norm` is a
//              minimum over timestamps of per-timestamp sums of squares of a time-aligned difference.  Row 0: the sum over the
//              feet of dx^2 + dy^2 of the relative positions; row 1: the sum of angle_distance(yaw, yaw_reference)^2.
//   motors     `motor_ring [max_stack][B]`: the sum over the motors of (q - q_reference)^2.
// A shift is the square root of the minimum over the first min(count + 1, max_stack) slots.  The minimum propagates NaN like
// `np.min` (`fmin_` would drop it), the sums like `np.sum`.  The slot differs from lane to lane, because lanes restart at
// different times: a store is a per-lane address, a reduction a plan-uniform loop over the rows with the lane's own bound as
// a predicate, and the row just written is taken from the register.  No launch argument changes from step to step.
//
// Caps: TRK_MAX_STACK = 1024 slots per family (the traffic of one launch), TRK_MAX_REL = 63 relative feet, TRK_MAX_MOTORS = 256.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "jm_locomotion.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [max_stack_odom, max_stack_foot, max_stack_motor, n_rel, n_motors]; `dt` (float64) is
// one unused entry (the plan has no real table; the upload takes no empty array).
constexpr int TRK_HEAD_INTS = 5;
constexpr int TRK_MAX_STACK = 1024;
constexpr int TRK_MAX_REL = 63;
constexpr int TRK_MAX_MOTORS = 256;
// launch modes
constexpr int TRK_RESTART = 0, TRK_PUSH = 1;
// rows of the `scalars` output
constexpr int TRK_DRIFT_POSITION = 0, TRK_DRIFT_ORIENTATION = 1, TRK_REWARD_ODOM_POSE = 2, TRK_SHIFT_FOOT_POSITIONS = 3,
              TRK_SHIFT_FOOT_ORIENTATIONS = 4, TRK_SHIFT_MOTOR_POSITIONS = 5;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool tracking_pack(const jm_tracking_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_tracking_plan_create: ";
    if (!d) { why = who + "null description"; return false; }
    const std::string range = " out of range [2, " + std::to_string(TRK_MAX_STACK) + "] (0: the family is absent)";
    const int32_t stacks[3] = {d->max_stack_odom, d->max_stack_foot, d->max_stack_motor};
    const char * names[3] = {"max_stack_odom ", "max_stack_foot ", "max_stack_motor "};
    for (int k = 0; k < 3; ++k)
        if (stacks[k] != 0 && (stacks[k] < 2 || stacks[k] > TRK_MAX_STACK))
        { why = who + names[k] + std::to_string(stacks[k]) + range; return false; }
    if (!d->max_stack_odom && !d->max_stack_foot && !d->max_stack_motor)
    { why = who + "no family: give at least one max_stack"; return false; }
    if (d->max_stack_foot && (d->n_rel < 1 || d->n_rel > TRK_MAX_REL))
    { why = who + "bad sizes (1 <= n_rel <= " + std::to_string(TRK_MAX_REL) + ": the feet but the last)"; return false; }
    if (d->max_stack_motor && (d->n_motors < 1 || d->n_motors > TRK_MAX_MOTORS))
    { why = who + "bad sizes (1 <= n_motors <= " + std::to_string(TRK_MAX_MOTORS) + ")"; return false; }
    if ((!d->max_stack_foot && d->n_rel != 0) || (!d->max_stack_motor && d->n_motors != 0))
    { why = who + "sizes of an absent family must be 0"; return false; }
    it = {d->max_stack_odom, d->max_stack_foot, d->max_stack_motor, d->n_rel, d->n_motors};
    dt = {0.0};
    return true;
}

// the inputs, the state and the outputs of one launch (device pointers of the kernel's scalar type but the two integer
// arrays); every one may be null
template<class T> struct TrkIO
{
    const T * odom_pose;                   // [3][B] x, y, yaw
    const T * reference_odom_pose;         // [3][B]
    const T * relative_pose;               // [7][R][B]
    const T * reference_relative_pose;     // [7][R][B]
    const T * position;                    // [M][B] joint side
    const T * reference_position;          // [M][B]
    const uint8_t * lane_mask;             // [B]
    int32_t * count;                       // [B]
    T * odom_ring;                         // [max_stack_odom][4][B]
    T * yaw_prev;                          // [2][B]
    T * yaw_ring;                          // [max_stack_odom - 1][2][B]
    T * foot_ring;                         // [2][max_stack_foot][B]
    T * motor_ring;                        // [max_stack_motor][B]
    T * delta_odom; T * delta_odom_reference;      // [3][B] each
    T * scalars;                           // [6][B]
};

// `angle_difference` (quantities/locomotion.py:1625-1627)
template<class T> JM_DEV T trk_angle_difference(T left, T right)
{
    const T pi = T(3.14159265358979323846);
    T delta = left - right;
    delta -= floor_((delta + pi) / (T(2) * pi)) * (T(2) * pi);
    return delta;
}

// `angle_distance` (compositions/locomotion.py:808-810)
template<class T> JM_DEV T trk_angle_distance(T left, T right)
{
    const T pi = T(3.14159265358979323846);
    T delta = left - right;
    delta -= floor_(delta / (T(2) * pi)) * (T(2) * pi);
    return pi - fabs_(delta - pi);
}

// `quat_to_yaw` (utils/math.py:103-104, 140-141) of rows 3-6 of column `j` of a `[7][R][B]` pose
template<class T> JM_DEV T trk_pose_yaw(const T * __restrict__ pose, int j, long long RB, long long B, long long lane)
{
    const long long o = (long long)j * B + lane;
    const T x = pose[3 * RB + o], y = pose[4 * RB + o], z = pose[5 * RB + o], w = pose[6 * RB + o];
    const T q_xy = y * x, q_yy = y * y, q_zz = z * z, q_zw = z * w;
    return atan2_(T(2) * (q_xy + q_zw), T(1) - T(2) * (q_yy + q_zz));
}

// `StackedQuantity.refresh`, wrapping array (quantities/transform.py:226-246), and `np.min` over the slots in use: `value` goes
// into slot count % max_stack of `ring [max_stack][B]`; returns the minimum of the first min(count + 1, max_stack) slots,
// NaN when one of them is.
template<class T> JM_DEV T trk_push_min(T * __restrict__ ring, int max_stack, int count, T value, long long B, long long lane)
{
    const int slot = (int)((unsigned)count % (unsigned)max_stack);      // (inside the ring whatever the counter holds)
    const int n = count + 1 < max_stack ? count + 1 : max_stack;
    ring[(long long)slot * B + lane] = value;
    T least = slot == 0 ? value : ring[lane];
    for (int k = 1; k < max_stack; ++k)
        if (k < n)
        {
            const T x = k == slot ? value : ring[(long long)k * B + lane];
            least = (x < least || x != x) ? x : least;
        }
    return least;
}

// The variation (x, y, yaw) of one odometry pose (`s` 0: true, 1: reference) over the window, and its state.
template<class T>
JM_DEV V3<T> trk_odom_delta(const TrkIO<T> & io, const T * __restrict__ pose, int s, int max_stack, int count, int mode, long long B,
                            long long lane)
{
    const T x = pose[lane], y = pose[B + lane], yaw = pose[2 * B + lane];
    // `DeltaQuantity.refresh`, bounds_only (quantities/transform.py:830): newest - oldest of the non-wrapping stack
    // (:247-254), kept as a ring
    const int slot = (int)((unsigned)count % (unsigned)max_stack);
    const int oldest = count + 1 >= max_stack ? (int)((unsigned)(count + 1) % (unsigned)max_stack) : 0;
    T * newest = io.odom_ring + ((long long)slot * 4 + 2 * s) * B + lane;
    const T * first = io.odom_ring + ((long long)oldest * 4 + 2 * s) * B + lane;
    newest[0] = x; newest[B] = y;
    V3<T> delta;
    delta.x = x - (oldest == slot ? x : first[0]);
    delta.y = y - (oldest == slot ? y : first[B]);
    // the inner `DeltaQuantity(horizon=None, op=angle_difference)`: op(newest, oldest) of a stack of two values, of one value
    // at the first step; then `quantity_stack.sum(axis=-1)` of the wrapping array of max_stack - 1 slots (:803-811, :831)
    const int yaw_stack = max_stack - 1;
    const int yaw_slot = (int)((unsigned)count % (unsigned)yaw_stack);
    const int yaw_n = count + 1 < yaw_stack ? count + 1 : yaw_stack;
    const T previous = mode == TRK_RESTART ? yaw : io.yaw_prev[s * B + lane];
    const T step = trk_angle_difference(yaw, previous);
    io.yaw_prev[s * B + lane] = yaw;
    io.yaw_ring[((long long)yaw_slot * 2 + s) * B + lane] = step;
    T sum = T(0);
    for (int k = 0; k < yaw_stack; ++k)
        if (k < yaw_n) sum += k == yaw_slot ? step : io.yaw_ring[((long long)k * 2 + s) * B + lane];
    delta.z = sum;
    return delta;
}

// All windows of one lane.  A family whose plan entry is 0 or one of whose inputs or state arrays is null is skipped;
// without `count` nothing runs.
template<class T>
JM_DEV void tracking_lane(const int32_t * __restrict__ it, const TrkIO<T> & io, int mode, T odometry_cutoff, long long B, long long lane)
{
    const int stack_o = it[0], stack_f = it[1], stack_m = it[2], R = it[3], M = it[4];
    if (!io.count) return;
    // the `num_steps` of every stack of the lane
    const int count = mode == TRK_RESTART ? 0 : io.count[lane] + 1;
    io.count[lane] = count;

    if (stack_o > 0 && io.odom_pose && io.reference_odom_pose && io.odom_ring && io.yaw_prev && io.yaw_ring)
    {
        const V3<T> d_true = trk_odom_delta(io, io.odom_pose, 0, stack_o, count, mode, B, lane);
        const V3<T> d_ref = trk_odom_delta(io, io.reference_odom_pose, 1, stack_o, count, mode, B, lane);
        if (io.delta_odom) { io.delta_odom[lane] = d_true.x; io.delta_odom[B + lane] = d_true.y; io.delta_odom[2 * B + lane] = d_true.z; }
        if (io.delta_odom_reference)
        { io.delta_odom_reference[lane] = d_ref.x; io.delta_odom_reference[B + lane] = d_ref.y; io.delta_odom_reference[2 * B + lane] = d_ref.z; }
        if (io.scalars)
        {
            // `compute_drift_error` (compositions/generic.py:205-208)
            const T ex = d_true.x - d_ref.x, ey = d_true.y - d_ref.y, eyaw = d_true.z - d_ref.z;
            io.scalars[(long long)TRK_DRIFT_POSITION * B + lane] = sqrt_(ex * ex + ey * ey);
            io.scalars[(long long)TRK_DRIFT_ORIENTATION * B + lane] = fabs_(eyaw);
            // `DriftTrackingBaseOdometryPoseReward` (compositions/locomotion.py:107-120): `l2_norm` of the position deltas
            if (odometry_cutoff > T(0))
            {
                const T en = sqrt_(d_true.x * d_true.x + d_true.y * d_true.y) - sqrt_(d_ref.x * d_ref.x + d_ref.y * d_ref.y);
                io.scalars[(long long)TRK_REWARD_ODOM_POSE * B + lane] = loco_rbf(en * en + eyaw * eyaw, odometry_cutoff);
            }
        }
    }

    if (stack_f > 0 && io.relative_pose && io.reference_relative_pose && io.foot_ring)
    {
        const long long RB = (long long)R * B;
        // the sums of squares of one timestamp, in the row order of `min_norm` (compositions/generic.py:328-330)
        T sq_position = T(0), sq_orientation = T(0);
        for (int c = 0; c < 2; ++c)
            for (int j = 0; j < R; ++j)
            {
                const long long o = c * RB + (long long)j * B + lane;
                const T e = io.relative_pose[o] - io.reference_relative_pose[o];
                sq_position += e * e;
            }
        for (int j = 0; j < R; ++j)
        {
            const T e = trk_angle_distance(trk_pose_yaw(io.relative_pose, j, RB, B, lane),
                                           trk_pose_yaw(io.reference_relative_pose, j, RB, B, lane));
            sq_orientation += e * e;
        }
        const T least_position = trk_push_min(io.foot_ring, stack_f, count, sq_position, B, lane);
        const T least_orientation = trk_push_min(io.foot_ring + (long long)stack_f * B, stack_f, count, sq_orientation, B, lane);
        if (io.scalars)
        {
            io.scalars[(long long)TRK_SHIFT_FOOT_POSITIONS * B + lane] = sqrt_(least_position);
            io.scalars[(long long)TRK_SHIFT_FOOT_ORIENTATIONS * B + lane] = sqrt_(least_orientation);
        }
    }

    if (stack_m > 0 && io.position && io.reference_position && io.motor_ring)
    {
        T sq = T(0);
        for (int m = 0; m < M; ++m)
        {
            const T e = io.position[(long long)m * B + lane] - io.reference_position[(long long)m * B + lane];
            sq += e * e;
        }
        const T least = trk_push_min(io.motor_ring, stack_m, count, sq, B, lane);
        if (io.scalars) io.scalars[(long long)TRK_SHIFT_MOTOR_POSITIONS * B + lane] = sqrt_(least);
    }
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_tracking(const int32_t * __restrict__ it, const TrkIO<T> io, int mode, double odometry_cutoff,
                                                   long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    tracking_lane<T>(it, io, mode, (T)odometry_cutoff, B, lane);
}
#endif
}  // namespace jm
