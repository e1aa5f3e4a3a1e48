// jm_actuation.h -- the actuated-joint quantities of the reference's quantity layer as one batched HIP kernel: position,
// velocity and acceleration of the actuated joints in motor order (joint or motor side), their distances to the mechanical
// stops, the count of motors about to hit a stop at speed, the instantaneous mechanical power, its average over a sliding
// window of environment steps and the reward on that average.  Every lane is one environment, arrays are `[rows][B]` like the
// physics state.  Everything is read from what a step left in device memory: `q`, `v`, `a` and `command`.
//
// Reference (python/gym_jiminy/common/gym_jiminy/common, restated per lane, operation for operation):
//   MultiActuatedJointKinematic.refresh           quantities/generic.py:1675-1691
//   compute_power, EnergyGenerationMode           quantities/generic.py:1694-1746
//   AverageMechanicalPowerConsumption             quantities/generic.py:1819-1887, over
//   StackedQuantity.refresh                       quantities/transform.py:208-296 (is_wrapping=True, as_array=True) and
//   mean = np.sum / size                          utils/math.py:18-33
//   _MultiActuatedJointBoundDistance.refresh      compositions/generic.py:500-502
//   MechanicalSafetyTermination.compute           compositions/generic.py:585-595
//   MinimizeMechanicalPowerConsumption            compositions/generic.py:153-191: radial_basis_function(average, cutoff, 2)
//                                                 (compositions/mixin.py:17-66; `loco_rbf` of jm_locomotion.h)
//
// All lanes interpret the same plan tables: their reads are indexed by loop counters only and become scalar loads.  Every
// mode of `compute_power` is a running sum, so a lane keeps no array.
//
// The sliding window is the first state of the quantity layer that survives environment steps.  It lives in two arrays the
// caller owns, `power_ring [max_stack][B]` and `power_count [B]` (the `num_steps` of the reference's stack, per lane), and the
// launch has two modes: ACT_RESTART (count = 0, slot 0 = the current power, the average is that value) and ACT_PUSH (count += 1,
// slot count % max_stack = the current power, the average over the first min(count + 1, max_stack) slots in storage order).
// The slot differs from lane to lane, because lanes restart at different times: the store is a per-lane address, the sum a
// plan-uniform loop over the rows with the lane's own bound as a predicate, and the row just written is taken from the
// register.  No running sum is kept (it would drift from `np.sum`), and no launch argument changes from step to step.
//
// Caps: ACT_MAX_MOTORS = 256 motors; ACT_MAX_STACK = 1024 slots: a launch reads `max_stack * B` scalars of the ring, so
// the cap bounds the traffic of one launch at 1024 rows (ten seconds of history at a 10 ms step).
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "jm_locomotion.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_motors, generator_mode, max_stack, n_motors x (idx_q, idx_v)];
// `dt` (float64) = [n_motors x (reduction, position_low, position_high)].
constexpr int ACT_HEAD_INTS = 3;
constexpr int ACT_MAX_MOTORS = 256;
constexpr int ACT_MAX_STACK = 1024;
// `EnergyGenerationMode` (quantities/generic.py:1694-1719)
constexpr int ACT_CHARGE = 0, ACT_LOST_EACH = 1, ACT_LOST_GLOBAL = 2, ACT_PENALIZE = 3;
// launch modes
constexpr int ACT_RESTART = 0, ACT_PUSH = 1;
// rows of the `scalars` output
constexpr int ACT_POWER = 0, ACT_POWER_AVERAGE = 1, ACT_REWARD_POWER = 2;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool actuation_pack(const jm_actuation_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_actuation_plan_create: ";
    if (!d) { why = who + "null description"; return false; }
    if (!d->idx_q || !d->idx_v || !d->reduction || !d->position_low || !d->position_high)
    { why = who + "null array in the description"; return false; }
    if (d->n_motors < 1 || d->n_motors > ACT_MAX_MOTORS)
    { why = who + "bad sizes (1 <= n_motors <= " + std::to_string(ACT_MAX_MOTORS) + ")"; return false; }
    if (d->nq < 1 || d->nv < 1) { why = who + "bad sizes (nq >= 1, nv >= 1)"; return false; }
    if (d->generator_mode < ACT_CHARGE || d->generator_mode > ACT_PENALIZE)
    { why = who + "generator_mode must be 0 CHARGE, 1 LOST_EACH, 2 LOST_GLOBAL or 3 PENALIZE"; return false; }
    if (d->max_stack < 2 || d->max_stack > ACT_MAX_STACK)
    { why = who + "max_stack " + std::to_string(d->max_stack) + " out of range [2, " + std::to_string(ACT_MAX_STACK) + "]"; return false; }
    for (int m = 0; m < d->n_motors; ++m)
    {
        const std::string at = "[" + std::to_string(m) + "]";
        if (d->idx_q[m] < 0 || d->idx_q[m] >= d->nq)
        { why = who + "idx_q" + at + " = " + std::to_string(d->idx_q[m]) + " out of range [0, " + std::to_string(d->nq) + ")"; return false; }
        if (d->idx_v[m] < 0 || d->idx_v[m] >= d->nv)
        { why = who + "idx_v" + at + " = " + std::to_string(d->idx_v[m]) + " out of range [0, " + std::to_string(d->nv) + ")"; return false; }
        if (!std::isfinite(d->reduction[m])) { why = who + "reduction" + at + " is not finite"; return false; }
        if (!std::isfinite(d->position_low[m]) || !std::isfinite(d->position_high[m]))
        { why = who + "the position bounds of motor " + std::to_string(m) + " are not finite"; return false; }
        if (d->position_low[m] > d->position_high[m])
        { why = who + "position_low" + at + " > position_high" + at; return false; }
    }
    it = {d->n_motors, d->generator_mode, d->max_stack};
    dt.clear();
    for (int m = 0; m < d->n_motors; ++m)
    {
        it.push_back(d->idx_q[m]); it.push_back(d->idx_v[m]);
        dt.push_back(d->reduction[m]); dt.push_back(d->position_low[m]); dt.push_back(d->position_high[m]);
    }
    return true;
}

// the inputs, the state and the outputs of one launch (device pointers of the kernel's scalar type but the three integer
// arrays); every one may be null
template<class T> struct ActIO
{
    const T * q;               // [nq][B]
    const T * v;               // [nv][B]
    const T * a;               // [nv][B]
    const T * command;         // [M][B] motor efforts, motor order
    const uint8_t * lane_mask; // [B]
    T * position; T * velocity; T * acceleration;      // [M][B] each
    T * bound_low; T * bound_high;                     // [M][B] each
    int32_t * safety;          // [B]
    T * scalars;               // [3][B]
    T * power_ring;            // [max_stack][B]
    int32_t * power_count;     // [B]
};

// All quantities of one lane.  A part whose inputs or output are null is skipped.
template<class T>
JM_DEV void actuation_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, const ActIO<T> & io, int mode, bool motor_side,
                           T position_margin, T velocity_max, T power_cutoff, long long B, long long lane)
{
    const int M = it[0], generator_mode = it[1], max_stack = it[2];
    const int32_t * idx = it + ACT_HEAD_INTS;
    const bool want_safety = io.safety && io.q && io.v && !(velocity_max < T(0));
    const bool want_power = io.scalars && io.command && io.v;
    int unsafe = 0;
    T power = T(0);
    for (int m = 0; m < M; ++m)
    {
        const long long o = (long long)m * B + lane;
        const T ratio = (T)dt[3 * m];
        T vj = T(0);
        if (io.v)
        {
            vj = io.v[(long long)idx[2 * m + 1] * B + lane];
            // `MultiActuatedJointKinematic.refresh` (:1685-1689): the row of the state, times the ratio on the motor side
            if (io.velocity) io.velocity[o] = motor_side ? vj * ratio : vj;
        }
        if (io.a && io.acceleration)
        {
            const T aj = io.a[(long long)idx[2 * m + 1] * B + lane];
            io.acceleration[o] = motor_side ? aj * ratio : aj;
        }
        if (io.q)
        {
            const T qj = io.q[(long long)idx[2 * m] * B + lane];
            if (io.position) io.position[o] = motor_side ? qj * ratio : qj;
            // `_MultiActuatedJointBoundDistance.refresh` (compositions/generic.py:500-502): joint side, whatever the flag
            const T low = qj - (T)dt[3 * m + 1], high = (T)dt[3 * m + 2] - qj;
            if (io.bound_low) io.bound_low[o] = low;
            if (io.bound_high) io.bound_high[o] = high;
            // `MechanicalSafetyTermination.compute` (:589-594), strict inequalities
            if (want_safety)
                unsafe += (int)(((low < position_margin) && (vj < -velocity_max)) || ((high < position_margin) && (vj > velocity_max)));
        }
        if (want_power)
        {
            // `compute_power` (quantities/generic.py:1738-1746) of the efforts and the motor-side velocities
            T p = (vj * ratio) * io.command[o];
            if (generator_mode == ACT_LOST_EACH) p = p < T(0) ? T(0) : p;
            else if (generator_mode == ACT_PENALIZE) p = fabs_(p);
            power += p;
        }
    }
    if (want_safety) io.safety[lane] = unsafe;
    if (!want_power) return;
    if (generator_mode == ACT_LOST_GLOBAL) power = power < T(0) ? T(0) : power;
    io.scalars[(long long)ACT_POWER * B + lane] = power;
    if (!io.power_ring || !io.power_count) return;

    // `StackedQuantity.refresh`, wrapping array (quantities/transform.py:226-246, 292), `mean` (utils/math.py:33)
    const int count = mode == ACT_RESTART ? 0 : io.power_count[lane] + 1;
    const int slot = (int)((unsigned)count % (unsigned)max_stack);      // (inside the ring whatever the counter holds)
    const int n = count + 1 < max_stack ? count + 1 : max_stack;
    io.power_count[lane] = count;
    io.power_ring[(long long)slot * B + lane] = power;
    T sum = T(0);
    for (int k = 0; k < max_stack; ++k)
        if (k < n) sum += k == slot ? power : io.power_ring[(long long)k * B + lane];
    const T average = sum / (T)n;
    io.scalars[(long long)ACT_POWER_AVERAGE * B + lane] = average;
    // `MinimizeMechanicalPowerConsumption` (compositions/generic.py:186-189)
    if (power_cutoff > T(0)) io.scalars[(long long)ACT_REWARD_POWER * B + lane] = loco_rbf(average * average, power_cutoff);
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_actuation(const int32_t * __restrict__ it, const double * __restrict__ dt, const ActIO<T> io, int mode,
                                                    int motor_side, double position_margin, double velocity_max, double power_cutoff,
                                                    long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    actuation_lane<T>(it, dt, io, mode, motor_side != 0, (T)position_margin, (T)velocity_max, (T)power_cutoff, B, lane);
}
#endif
}  // namespace jm
