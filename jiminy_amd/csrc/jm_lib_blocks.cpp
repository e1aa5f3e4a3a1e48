// jm_lib_blocks.cpp -- the part of the C ABI (include/jiminy_hip.h) that does not depend on the topology:
//   * the per-tick pipeline blocks and the sensor / model-bias blocks (`jm_block_*` without a plan);
//   * the plan-backed blocks: `jm_<family>_plan_create / _destroy` and the launches behind them, for the families deform,
//     attitude, frames, locomotion, actuation, footposes, tracking, trajectory, centroidal, trackrewards, support, compose
//     and observe (one `jm_<family>.h` each holds the pack function and the kernel);
//   * the seeding of the generators.
// Compiled with the flags of jm_lib.cpp and linked into every topology library (jiminy_amd/codegen.py), in a translation
// unit of its own so that the physics kernels of jm_lib.cpp are compiled without it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <random>
#include <string>
#include <vector>

#include "jm_blocks.h"
#include "jm_deform.h"
#include "jm_attitude.h"
#include "jm_frames.h"
#include "jm_locomotion.h"
#include "jm_actuation.h"
#include "jm_footposes.h"
#include "jm_tracking.h"
#include "jm_trajectory.h"
#include "jm_centroidal.h"
#include "jm_trackrewards.h"
#include "jm_support.h"
#include "jm_compose.h"
#include "jm_observe.h"
#include "jm_random.h"
#include "jm_error.h"

namespace
{
// The dtype switch and the launch of a one-thread-per-lane kernel: `launch(z, grid, s)` receives a zero of the scalar
// type (like `with_dtype` of jm_lib.cpp), the grid of (B + 255) / 256 x `grid_y` blocks of 256 threads and the stream.
template<class F> int32_t launch_lanes(int32_t dtype, int64_t B, unsigned grid_y, void * stream, F && launch)
{
    const dim3 grid((unsigned)((B + 255) / 256), grid_y);
    if (dtype == JM_F64) launch(double(), grid, (hipStream_t)stream);
    else launch(float(), grid, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return JM_OK;
}

// the two packed arrays of a plan (jm_deform.h, jm_attitude.h) on the device
struct DevicePlan
{
    int32_t * it = nullptr;
    double * dt = nullptr;
    hipError_t upload(const std::vector<int32_t> & h_it, const std::vector<double> & h_dt)
    {
        hipError_t e = hipMalloc((void **)&it, h_it.size() * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc((void **)&dt, h_dt.size() * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(it, h_it.data(), h_it.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dt, h_dt.data(), h_dt.size() * sizeof(double), hipMemcpyHostToDevice);
        return e;
    }
    ~DevicePlan()
    {
        if (it) (void)hipFree(it);
        if (dt) (void)hipFree(dt);
    }
};

// validate and pack a description (`pack`), upload it into a new `Plan`
template<class Plan, class Desc, class Pack> int32_t plan_create(const std::string & who, const Desc * desc, Plan ** out, Pack pack)
{
    if (!out) return fail(JM_EINVAL, who + ": null argument");
    *out = nullptr;
    std::vector<int32_t> it;
    std::vector<double> dt;
    std::string why;
    if (!pack(desc, it, dt, why)) return fail(JM_EINVAL, why);
    Plan * p = new (std::nothrow) Plan;
    if (!p) return fail(JM_ERUNTIME, "out of host memory");
    const hipError_t e = p->dev.upload(it, dt);
    if (e != hipSuccess)
    {
        delete p;
        return fail(JM_ERUNTIME, who + ": " + hipGetErrorString(e));
    }
    *out = p;
    return JM_OK;
}
// what every plan holds; a family with more state adds members
struct PlanBase
{
    DevicePlan dev;
};

template<class Plan> int32_t plan_destroy(Plan * p)
{
    delete p;
    return JM_OK;
}

// the checks every launch starts with, in this order: a null argument (`given` false), a bad size (`sizes_ok` false), a dtype
// that is neither JM_F64 nor JM_F32.  JM_OK when all pass; the message is built on failure only.
int32_t check_call(const char * who, bool given, bool sizes_ok, int32_t dtype)
{
    const char * what = !given ? ": null argument" : !sizes_ok ? ": bad sizes" : (dtype != JM_F64 && dtype != JM_F32) ? ": bad dtype" : nullptr;
    return what ? fail(JM_EINVAL, std::string(who) + what) : JM_OK;
}

// the pointers of a `jm_locomotion_io` in the scalar type of the launch (the ground members keep their defaults)
template<class T> jm::LocoIO<T> loco_io(const jm_locomotion_io * io)
{
    return {(const T *)io->centroidal, (const T *)io->q_root, (const T *)io->model_lane, (const T *)io->con_lambda,
            io->con_flags, (const T *)io->v_avg, (const T *)io->quat_no_yaw, (const T *)io->pose, io->lane_mask,
            (T *)io->com, (T *)io->vcom, (T *)io->odom_pose, (T *)io->zmp, (T *)io->dcm, (T *)io->h_angular,
            (T *)io->contact_force_rel, (T *)io->foot_force_vertical, (T *)io->scalars};
}
}  // namespace

// ---- the opaque plan types of include/jiminy_hip.h: validated, packed and uploaded once; every call is one launch
struct jm_deform_plan : PlanBase
{
    int n_imu = 0, n_flex = 0, ignore_twist = 0;
};
struct jm_attitude_plan : PlanBase
{
    int n_imu = 0;
};
struct jm_frames_plan : PlanBase {};
struct jm_locomotion_plan : PlanBase {};
struct jm_actuation_plan : PlanBase {};
struct jm_footposes_plan : PlanBase {};
struct jm_tracking_plan : PlanBase {};
struct jm_centroidal_plan : PlanBase {};
struct jm_trackrewards_plan : PlanBase {};
struct jm_support_plan : PlanBase {};
struct jm_compose_plan : PlanBase {};
// the reference trajectories: the samples `[S][R]` in the plan's dtype next to the tables
struct jm_trajectory_plan : PlanBase
{
    void * data = nullptr;
    int32_t dtype = 0;
    ~jm_trajectory_plan()
    {
        if (data) (void)hipFree(data);
    }
};
// the observation assembly: the integer table stays on the host as well, for the aliasing check of a launch
struct jm_observe_plan : PlanBase
{
    std::vector<int32_t> it;
};

extern "C"
{
int32_t jm_block_pd_controller(int32_t dtype, int64_t B, int32_t M, const void * encoder,
                               const int32_t * encoder_index, void * command_state, const double * lower,
                               const double * upper, const double * kp, const double * kd,
                               const double * effort_limit, double control_dt, void * out_torque, void * stream)
{
    if (!encoder || !encoder_index || !command_state || !lower || !upper || !kp || !kd || !effort_limit || !out_torque)
        return fail(JM_EINVAL, "jm_block_pd_controller: null argument");
    if (B <= 0 || M <= 0 || M > JM_BLOCK_MAX_MOTORS) return fail(JM_EINVAL, "jm_block_pd_controller: bad sizes");
    if (control_dt < 0.0) return fail(JM_EINVAL, "Integration backward in time is not supported.");
    if (dtype != JM_F64 && dtype != JM_F32) return fail(JM_EINVAL, "jm_block_pd_controller: bad dtype");
    jm::PdParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = M;
    p.dt = control_dt;
    for (int m = 0; m < M; ++m)
    {
        p.enc_index[m] = encoder_index[m];
        for (int k = 0; k < 3; ++k) { p.lo[k][m] = lower[k * M + m]; p.hi[k][m] = upper[k * M + m]; }
        p.kp[m] = kp[m]; p.kd[m] = kd[m]; p.effort_limit[m] = effort_limit[m];
    }
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_pd_controller<T>), grid, dim3(256), 0, s, p, (const T *)encoder,
                           (T *)command_state, (T *)out_torque, (long long)B);
    });
}

int32_t jm_block_mahony_filter(int32_t dtype, int64_t B, int32_t n_imu, const void * imu, void * quat, void * omega,
                               void * cf, void * bias, double kp, double ki, double dt, void * stream)
{
    if (const int32_t rc = check_call("jm_block_mahony_filter", imu && quat && omega && cf && bias, B > 0 && n_imu > 0, dtype)) return rc;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_mahony<T>), grid, dim3(256), 0, s, n_imu, (const T *)imu, (T *)quat,
                           (T *)omega, (T *)cf, (T *)bias, kp, ki, dt, (long long)B);
    });
}

int32_t jm_block_pd_adapter(int32_t dtype, int64_t B, int32_t M, const void * action, int32_t order, void * command_state,
                            const double * lower, const double * upper, int32_t is_instantaneous, const double * velocity_deadband,
                            double step_dt, void * out, void * stream)
{
    if (!action || !command_state || !lower || !upper || !out) return fail(JM_EINVAL, "jm_block_pd_adapter: null argument");
    if (B <= 0 || M <= 0 || M > JM_BLOCK_MAX_MOTORS) return fail(JM_EINVAL, "jm_block_pd_adapter: bad sizes");
    if (order != 0 && order != 1) return fail(JM_EINVAL, "Derivative order of the target must be either 0 or 1.");
    if (dtype != JM_F64 && dtype != JM_F32) return fail(JM_EINVAL, "jm_block_pd_adapter: bad dtype");
    jm::PdAdapterParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = M; p.order = order; p.instantaneous = is_instantaneous != 0; p.dt = step_dt;
    for (int m = 0; m < M; ++m)
    {
        for (int k = 0; k < 3; ++k) { p.lo[k][m] = lower[k * M + m]; p.hi[k][m] = upper[k * M + m]; }
        p.deadband[m] = velocity_deadband ? velocity_deadband[m] : -1.0;
    }
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_pd_adapter<T>), grid, dim3(256), 0, s, p, (const T *)action, (T *)command_state,
                           (T *)out, (long long)B);
    });
}

int32_t jm_block_motor_safety_limit(int32_t dtype, int64_t B, int32_t M, const void * encoder, const int32_t * encoder_index,
                                    const void * command, const double * kp, const double * kd, const double * soft_lo,
                                    const double * soft_hi, const double * vel_lim, const double * eff_lim, void * out, void * stream)
{
    const bool given = encoder && encoder_index && command && kp && kd && soft_lo && soft_hi && vel_lim && eff_lim && out;
    if (const int32_t rc = check_call("jm_block_motor_safety_limit", given, B > 0 && M > 0 && M <= JM_BLOCK_MAX_MOTORS, dtype)) return rc;
    jm::SafetyParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = M;
    for (int m = 0; m < M; ++m)
    {
        p.enc_index[m] = encoder_index[m];
        p.kp[m] = kp[m]; p.kd[m] = kd[m]; p.soft_lo[m] = soft_lo[m]; p.soft_hi[m] = soft_hi[m];
        p.vel_lim[m] = vel_lim[m]; p.eff_lim[m] = eff_lim[m];
    }
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_motor_safety_limit<T>), grid, dim3(256), 0, s, p, (const T *)encoder,
                           (const T *)command, (T *)out, (long long)B);
    });
}

int32_t jm_deform_plan_create(const jm_deform_desc * desc, jm_deform_plan ** out)
{
    const int32_t rc = plan_create("jm_deform_plan_create", desc, out, jm::deform_pack);
    if (rc != JM_OK) return rc;
    (*out)->n_imu = desc->n_imu; (*out)->n_flex = desc->n_flex; (*out)->ignore_twist = desc->ignore_twist != 0;
    return JM_OK;
}

int32_t jm_deform_plan_destroy(jm_deform_plan * p) { return plan_destroy(p); }

int32_t jm_block_deformation_estimator(const jm_deform_plan * p, int32_t dtype, int64_t B, const void * encoder,
                                       const void * imu_quat, void * out_quat, void * out_rpy, void * stream)
{
    if (const int32_t rc = check_call("jm_block_deformation_estimator", p && encoder && imu_quat && out_quat, B > 0, dtype)) return rc;
    const jm::DeformArgs a{p->dev.it, p->dev.dt, p->n_imu, p->n_flex, p->ignore_twist};
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_deformation_estimator<T>), grid, dim3(256), 0, s, a, (const T *)encoder,
                           (const T *)imu_quat, (T *)out_quat, (T *)out_rpy, (long long)B);
    });
}

int32_t jm_attitude_plan_create(const jm_attitude_desc * desc, jm_attitude_plan ** out)
{
    const int32_t rc = plan_create("jm_attitude_plan_create", desc, out, jm::attitude_pack);
    if (rc != JM_OK) return rc;
    (*out)->n_imu = desc->n_imu;
    return JM_OK;
}

int32_t jm_attitude_plan_destroy(jm_attitude_plan * p) { return plan_destroy(p); }

int32_t jm_block_attitude_init(const jm_attitude_plan * p, int32_t dtype, int64_t B, const void * q, const void * imu,
                               const uint8_t * lane_mask, int32_t exact_init, void * quat, void * omega, void * cf, void * bias,
                               void * twist, void * rpy, void * stream)
{
    if (const int32_t rc = check_call("jm_block_attitude_init", p && q && imu && quat && omega && cf && bias, B > 0, dtype)) return rc;
    const jm::AttitudeArgs a{p->dev.it, p->dev.dt, p->n_imu};
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_attitude_init<T>), grid, dim3(256), 0, s, a, (int)(exact_init != 0), (const T *)q,
                           (const T *)imu, lane_mask, (T *)quat, (T *)omega, (T *)cf, (T *)bias,
                           (T *)twist, (T *)rpy, (long long)B);
    });
}

int32_t jm_block_mahony_observer(const jm_attitude_plan * p, int32_t dtype, int64_t B, const void * imu, void * quat, void * omega,
                                 void * cf, void * bias, double dt, int32_t ignore_twist, void * rpy, void * stream)
{
    if (const int32_t rc = check_call("jm_block_mahony_observer", p && imu && quat && omega && cf && bias, B > 0, dtype)) return rc;
    const jm::AttitudeArgs a{p->dev.it, p->dev.dt, p->n_imu};
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_mahony_observer<T>), grid, dim3(256), 0, s, a, (const T *)imu, (T *)quat,
                           (T *)omega, (T *)cf, (T *)bias, dt, (int)(ignore_twist != 0), (T *)rpy, (long long)B);
    });
}

int32_t jm_block_body_observer(const jm_attitude_plan * p, int32_t dtype, int64_t B, const void * imu_quat, const void * imu_omega,
                               void * quat, void * omega, void * twist, int32_t twist_mode, double time_constant_inv, double dt,
                               void * rpy, void * stream)
{
    if (const int32_t rc = check_call("jm_block_body_observer", p && imu_quat && imu_omega && quat && omega, B > 0, dtype)) return rc;
    if (twist_mode < 0 || twist_mode > 2) return fail(JM_EINVAL, "jm_block_body_observer: twist_mode must be 0, 1 or 2");
    if (twist_mode == 2 && !twist) return fail(JM_EINVAL, "jm_block_body_observer: twist_mode 2 needs the twist state");
    if (quat == imu_quat) return fail(JM_EINVAL, "jm_block_body_observer: quat must not alias imu_quat");
    const jm::AttitudeArgs a{p->dev.it, p->dev.dt, p->n_imu};
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_body_observer<T>), grid, dim3(256), 0, s, a, (const T *)imu_quat,
                           (const T *)imu_omega, (T *)quat, (T *)omega, (T *)twist, (int)twist_mode,
                           time_constant_inv, dt, (T *)rpy, (long long)B);
    });
}

int32_t jm_frames_plan_create(const jm_frames_desc * desc, jm_frames_plan ** out)
{
    return plan_create("jm_frames_plan_create", desc, out, jm::frames_pack);
}

int32_t jm_frames_plan_destroy(jm_frames_plan * p) { return plan_destroy(p); }

int32_t jm_block_frame_kinematics(const jm_frames_plan * p, int32_t dtype, int64_t B, const void * q, const void * v,
                                  const void * model_lane, const uint8_t * lane_mask, void * pose, void * pose_prev, void * rpy,
                                  void * vel, void * stream)
{
    if (!p || !q) return fail(JM_EINVAL, "jm_block_frame_kinematics: null argument");
    if (vel && !v) return fail(JM_EINVAL, "jm_block_frame_kinematics: the frame velocity needs v");
    if (B <= 0) return fail(JM_EINVAL, "jm_block_frame_kinematics: bad sizes");
    if (dtype != JM_F64 && dtype != JM_F32) return fail(JM_EINVAL, "jm_block_frame_kinematics: bad dtype");
    if (pose && pose == pose_prev) return fail(JM_EINVAL, "jm_block_frame_kinematics: pose_prev must not alias pose");
    const jm::FramesArgs a{p->dev.it, p->dev.dt};
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_frame_kinematics<T>), grid, dim3(256), 0, s, a, (const T *)q, (const T *)v,
                           (const T *)model_lane, lane_mask, (T *)pose, (T *)pose_prev, (T *)rpy, (T *)vel, (long long)B);
    });
}

int32_t jm_block_frame_average(const jm_frames_plan * p, int32_t dtype, int64_t B, void * pose_prev, const void * pose,
                               double inv_step_dt, void * v_avg, void * pose_mean, void * quat_no_yaw, void * stream)
{
    if (const int32_t rc = check_call("jm_block_frame_average", p && pose_prev && pose, B > 0, dtype)) return rc;
    if (pose_prev == pose) return fail(JM_EINVAL, "jm_block_frame_average: pose_prev must not alias pose");
    const jm::FramesArgs a{p->dev.it, p->dev.dt};
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_frame_average<T>), grid, dim3(256), 0, s, a, (T *)pose_prev, (const T *)pose, inv_step_dt,
                           (T *)v_avg, (T *)pose_mean, (T *)quat_no_yaw, (long long)B);
    });
}

int32_t jm_locomotion_plan_create(const jm_locomotion_desc * desc, jm_locomotion_plan ** out)
{
    return plan_create("jm_locomotion_plan_create", desc, out, jm::locomotion_pack);
}

int32_t jm_locomotion_plan_destroy(jm_locomotion_plan * p) { return plan_destroy(p); }

int32_t jm_block_locomotion(const jm_locomotion_plan * p, int32_t dtype, int64_t B, const jm_locomotion_io * io,
                            double momentum_cutoff, double friction_cutoff, void * stream)
{
    if (const int32_t rc = check_call("jm_block_locomotion", p && io, B > 0, dtype)) return rc;
    const int32_t * it = p->dev.it;
    const double * dt = p->dev.dt;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        const jm::LocoIO<T> a = loco_io<T>(io);
        hipLaunchKernelGGL((jm::k_locomotion<T>), grid, dim3(256), 0, s, it, dt, a, momentum_cutoff, friction_cutoff, (long long)B);
    });
}

int32_t jm_block_locomotion_ground(const jm_locomotion_plan * p, int32_t dtype, int64_t B, const jm_locomotion_io * io,
                                   const jm_locomotion_ground * g, double momentum_cutoff, double friction_cutoff, void * stream)
{
    if (const int32_t rc = check_call("jm_block_locomotion_ground", p && io, B > 0, dtype)) return rc;
    std::string why;
    if (!jm::locomotion_ground_check(g, io, why)) return fail(JM_EINVAL, why);
    const int32_t * it = p->dev.it;
    const double * dt = p->dev.dt;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        jm::LocoIO<T> a = loco_io<T>(io);
        if (!g || !g->heights)
        {
            // flat ground: the kernel of jm_block_locomotion itself, so that the outputs are equal bit for bit
            hipLaunchKernelGGL((jm::k_locomotion<T>), grid, dim3(256), 0, s, it, dt, a, momentum_cutoff, friction_cutoff, (long long)B);
            if (g && g->contact_ground)
                hipLaunchKernelGGL((jm::k_locomotion_flat_ground<T>), grid, dim3(256), 0, s, it, (T *)g->contact_ground, io->lane_mask,
                                   (long long)B);
            return;
        }
        a.ground_h = (const T *)g->heights; a.ground_nx = g->nx; a.ground_ny = g->ny;
        a.ground_x0 = (T)g->x0; a.ground_y0 = (T)g->y0; a.ground_dx = (T)g->dx; a.ground_dy = (T)g->dy;
        a.ground_off = (const T *)g->offsets;
        a.contact_ground = (T *)g->contact_ground;
        hipLaunchKernelGGL((jm::k_locomotion<T, true>), grid, dim3(256), 0, s, it, dt, a, momentum_cutoff, friction_cutoff, (long long)B);
    });
}

int32_t jm_actuation_plan_create(const jm_actuation_desc * desc, jm_actuation_plan ** out)
{
    return plan_create("jm_actuation_plan_create", desc, out, jm::actuation_pack);
}

int32_t jm_actuation_plan_destroy(jm_actuation_plan * p) { return plan_destroy(p); }

int32_t jm_block_actuation(const jm_actuation_plan * p, int32_t dtype, int64_t B, const jm_actuation_io * io, int32_t mode,
                           int32_t motor_side, double position_margin, double velocity_max, double power_cutoff, void * stream)
{
    if (const int32_t rc = check_call("jm_block_actuation", p && io, B > 0, dtype)) return rc;
    if (mode != jm::ACT_RESTART && mode != jm::ACT_PUSH) return fail(JM_EINVAL, "jm_block_actuation: mode must be 0 (restart) or 1 (push)");
    const int32_t * it = p->dev.it;
    const double * dt = p->dev.dt;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        const jm::ActIO<T> a{(const T *)io->q, (const T *)io->v, (const T *)io->a, (const T *)io->command, io->lane_mask,
                             (T *)io->position, (T *)io->velocity, (T *)io->acceleration, (T *)io->bound_low, (T *)io->bound_high,
                             io->safety, (T *)io->scalars, (T *)io->power_ring, io->power_count};
        hipLaunchKernelGGL((jm::k_actuation<T>), grid, dim3(256), 0, s, it, dt, a, (int)mode, (int)motor_side, position_margin,
                           velocity_max, power_cutoff, (long long)B);
    });
}

int32_t jm_footposes_plan_create(const jm_footposes_desc * desc, jm_footposes_plan ** out)
{
    return plan_create("jm_footposes_plan_create", desc, out, jm::footposes_pack);
}

int32_t jm_footposes_plan_destroy(jm_footposes_plan * p) { return plan_destroy(p); }

int32_t jm_block_foot_poses(const jm_footposes_plan * p, int32_t dtype, int64_t B, const jm_footposes_io * io, double position_cutoff,
                            double orientation_cutoff, void * stream)
{
    if (const int32_t rc = check_call("jm_block_foot_poses", p && io, B > 0, dtype)) return rc;
    const int32_t * it = p->dev.it;
    const double * dt = p->dev.dt;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        const jm::FootIO<T> a{(const T *)io->pose, (const T *)io->reference_relative_pose, io->lane_mask, (T *)io->mean_pose,
                              (T *)io->mean_odom_pose, (T *)io->relative_pose, (T *)io->tracking_error, (T *)io->scalars};
        hipLaunchKernelGGL((jm::k_foot_poses<T>), grid, dim3(256), 0, s, it, dt, a, position_cutoff, orientation_cutoff, (long long)B);
    });
}

int32_t jm_tracking_plan_create(const jm_tracking_desc * desc, jm_tracking_plan ** out)
{
    return plan_create("jm_tracking_plan_create", desc, out, jm::tracking_pack);
}

int32_t jm_tracking_plan_destroy(jm_tracking_plan * p) { return plan_destroy(p); }

int32_t jm_block_tracking(const jm_tracking_plan * p, int32_t dtype, int64_t B, const jm_tracking_io * io, int32_t mode,
                          double odometry_cutoff, void * stream)
{
    if (const int32_t rc = check_call("jm_block_tracking", p && io, B > 0, dtype)) return rc;
    if (mode != jm::TRK_RESTART && mode != jm::TRK_PUSH) return fail(JM_EINVAL, "jm_block_tracking: mode must be 0 (restart) or 1 (push)");
    const int32_t * it = p->dev.it;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        const jm::TrkIO<T> a{(const T *)io->odom_pose, (const T *)io->reference_odom_pose, (const T *)io->relative_pose,
                             (const T *)io->reference_relative_pose, (const T *)io->position, (const T *)io->reference_position,
                             io->lane_mask, io->count, (T *)io->odom_ring, (T *)io->yaw_prev, (T *)io->yaw_ring, (T *)io->foot_ring,
                             (T *)io->motor_ring, (T *)io->delta_odom, (T *)io->delta_odom_reference, (T *)io->scalars};
        hipLaunchKernelGGL((jm::k_tracking<T>), grid, dim3(256), 0, s, it, a, (int)mode, odometry_cutoff, (long long)B);
    });
}

int32_t jm_trajectory_plan_create(const jm_trajectory_desc * desc, jm_trajectory_plan ** out)
{
    const int32_t rc = plan_create("jm_trajectory_plan_create", desc, out, jm::trajectory_pack);
    if (rc != JM_OK) return rc;
    jm_trajectory_plan * p = *out;
    p->dtype = desc->dtype;
    const size_t bytes = (size_t)desc->n_samples * (size_t)jm::trajectory_row_size(desc->nq, desc->nv, desc->n_command, desc->fields) *
                         (desc->dtype == JM_F64 ? sizeof(double) : sizeof(float));
    hipError_t e = hipMalloc(&p->data, bytes);
    if (e == hipSuccess) e = hipMemcpy(p->data, desc->data, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        delete p;
        *out = nullptr;
        return fail(JM_ERUNTIME, std::string("jm_trajectory_plan_create: ") + hipGetErrorString(e));
    }
    return JM_OK;
}

int32_t jm_trajectory_plan_destroy(jm_trajectory_plan * p) { return plan_destroy(p); }

int32_t jm_block_trajectory_state(const jm_trajectory_plan * p, int32_t dtype, int64_t B, const jm_trajectory_io * io, void * stream)
{
    if (const int32_t rc = check_call("jm_block_trajectory_state", p && io && io->time && io->trajectory && io->time_offset, B > 0, dtype)) return rc;
    if (dtype != p->dtype) return fail(JM_EINVAL, "jm_block_trajectory_state: dtype is not the one the plan was created with");
    const int32_t * it = p->dev.it;
    const double * dt = p->dev.dt;
    const void * data = p->data;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        const jm::TrajIO<T> a{io->time, io->trajectory, io->time_offset, io->lane_mask, (T *)io->q, (T *)io->v, (T *)io->a,
                              (T *)io->command, (T *)io->odom_pose, (T *)io->position, io->status};
        hipLaunchKernelGGL((jm::k_trajectory_state<T>), grid, dim3(256), 0, s, it, dt, (const T *)data, a, (long long)B);
    });
}

int32_t jm_centroidal_plan_create(const jm_centroidal_desc * desc, jm_centroidal_plan ** out)
{
    return plan_create("jm_centroidal_plan_create", desc, out, jm::centroidal_pack);
}

int32_t jm_centroidal_plan_destroy(jm_centroidal_plan * p) { return plan_destroy(p); }

int32_t jm_block_centroidal_state(const jm_centroidal_plan * p, int32_t dtype, int64_t B, const void * q, const void * v,
                                  const void * a, const uint8_t * lane_mask, void * centroidal, void * stream)
{
    if (const int32_t rc = check_call("jm_block_centroidal_state", p && q && v, B > 0, dtype)) return rc;
    if (!centroidal) return JM_OK;      // (the only output is absent: nothing is written)
    const jm::FramesArgs args{p->dev.it, p->dev.dt};
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_centroidal_state<T>), grid, dim3(256), 0, s, args, (const T *)q, (const T *)v, (const T *)a,
                           lane_mask, (T *)centroidal, (long long)B);
    });
}

int32_t jm_trackrewards_plan_create(const jm_trackrewards_desc * desc, jm_trackrewards_plan ** out)
{
    return plan_create("jm_trackrewards_plan_create", desc, out, jm::trackrewards_pack);
}

int32_t jm_trackrewards_plan_destroy(jm_trackrewards_plan * p) { return plan_destroy(p); }

int32_t jm_block_tracking_rewards(const jm_trackrewards_plan * p, int32_t dtype, int64_t B, const jm_trackrewards_io * io,
                                  const double * cutoff, void * stream)
{
    if (const int32_t rc = check_call("jm_block_tracking_rewards", p && io && cutoff, B > 0, dtype)) return rc;
    jm::TrkRewCutoffs c;
    for (int k = 0; k < jm::TR_TERMS; ++k) c.c[k] = cutoff[k] > 0.0 ? cutoff[k] : 0.0;     // (NaN: skipped as well)
    const int32_t * it = p->dev.it;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        const jm::TrkRewIO<T> a{(const T *)io->pose, (const T *)io->pose_reference, (const T *)io->v_avg, (const T *)io->quat_no_yaw,
                                (const T *)io->v_avg_reference, (const T *)io->quat_no_yaw_reference, (const T *)io->dcm,
                                (const T *)io->dcm_reference, (const T *)io->position, (const T *)io->position_reference, io->lane_mask,
                                (T *)io->value, (T *)io->reference, (T *)io->rewards};
        hipLaunchKernelGGL((jm::k_tracking_rewards<T>), grid, dim3(256), 0, s, it, a, c, (long long)B);
    });
}

int32_t jm_support_plan_create(const jm_support_desc * desc, jm_support_plan ** out)
{
    return plan_create("jm_support_plan_create", desc, out, jm::support_pack);
}

int32_t jm_support_plan_destroy(jm_support_plan * p) { return plan_destroy(p); }

int32_t jm_block_support_polygon(const jm_support_plan * p, int32_t dtype, int64_t B, const jm_support_io * io, double cutoff_inner,
                                 double cutoff_outer, void * stream)
{
    if (const int32_t rc = check_call("jm_block_support_polygon", p && io, B > 0, dtype)) return rc;
    std::string why;
    if (!jm::support_cutoffs_check(cutoff_inner, cutoff_outer, why)) return fail(JM_EINVAL, why);
    const int32_t * it = p->dev.it;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        const jm::SupportIO<T> a{(const T *)io->pose, (const T *)io->odom_pose, (const T *)io->zmp, io->lane_mask, io->n_vertices,
                                 io->vertex_index, (T *)io->vertices, (T *)io->center, (T *)io->scalars};
        hipLaunchKernelGGL((jm::k_support_polygon<T>), grid, dim3(256), 0, s, it, a, cutoff_inner, cutoff_outer, (long long)B);
    });
}

int32_t jm_compose_plan_create(const jm_compose_desc * desc, jm_compose_plan ** out)
{
    return plan_create("jm_compose_plan_create", desc, out, jm::compose_pack);
}

int32_t jm_compose_plan_destroy(jm_compose_plan * p) { return plan_destroy(p); }

int32_t jm_block_compose(const jm_compose_plan * p, int32_t dtype, int64_t B, const jm_compose_io * io, int32_t training, void * stream)
{
    if (const int32_t rc = check_call("jm_block_compose", p && io, B > 0, dtype)) return rc;
    const int32_t * it = p->dev.it;
    const double * dt = p->dev.dt;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        jm::ComposeIO<T> a;
        for (int k = 0; k < jm::CMP_MAX_SOURCES; ++k) a.source[k] = io->source[k];
        a.time = (const T *)io->time; a.base_terminated = io->base_terminated; a.base_truncated = io->base_truncated;
        a.lane_mask = io->lane_mask; a.reward = (T *)io->reward; a.node_value = (T *)io->node_value;
        a.terminated = io->terminated; a.truncated = io->truncated; a.trigger = io->trigger; a.violations = io->violations;
        hipLaunchKernelGGL((jm::k_compose<T>), grid, dim3(256), 0, s, it, dt, a, (int)(training != 0), (long long)B);
    });
}

// ≙ the constructors of `AdaptLayoutObservation` (observation_layout.py:394-429), `ScaleObservation` (scale.py:150-229),
// `NormalizeObservation` (normalize.py:49-90), `StackObservation` (observation_stack.py:40-160) and `FlattenObservation`
// (flatten.py), whose result the caller states as elements and positions
int32_t jm_observe_plan_create(const jm_observe_desc * desc, jm_observe_plan ** out)
{
    std::vector<int32_t> kept;
    const int32_t rc = plan_create("jm_observe_plan_create", desc, out,
                                   [&](const jm_observe_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why) {
                                       const bool ok = jm::observe_pack(d, it, dt, why);
                                       if (ok) kept = it;
                                       return ok;
                                   });
    if (rc == JM_OK) (*out)->it = std::move(kept);
    return rc;
}

int32_t jm_observe_plan_destroy(jm_observe_plan * p) { return plan_destroy(p); }

// ≙ one `transform_observation` of the whole chain: `_array_scale` per scale operation (scale.py:236-244), the affine map of
// normalize.py:92-114, the shift and the write of observation_stack.py:225-265 and the concatenation of flatten.py
int32_t jm_block_observe(const jm_observe_plan * p, int32_t dtype_in, int32_t dtype_out, int64_t B, const jm_observe_io * io, int32_t shift,
                         void * stream)
{
    if (!p || !io) return fail(JM_EINVAL, "jm_block_observe: null argument");
    if (B <= 0) return fail(JM_EINVAL, "jm_block_observe: bad sizes");
    std::string why;
    if (!jm::observe_dtype_check(dtype_in, dtype_out, why)) return fail(JM_EINVAL, why);
    if (!jm::observe_alias_check(p->it, io, B, dtype_in == JM_F64 ? 8 : 4, dtype_out == JM_F64 ? 8 : 4, why)) return fail(JM_EINVAL, why);
    const int32_t * it = p->dev.it;
    const double * dt = p->dev.dt;
    const dim3 grid((unsigned)((B + jm::OBS_TILE - 1) / jm::OBS_TILE), (unsigned)((p->it[1] + jm::OBS_TILE - 1) / jm::OBS_TILE));
    const auto launch = [&](auto zi, auto zo) {
        using TIn = decltype(zi);
        using TOut = decltype(zo);
        jm::ObserveIO<TIn, TOut> a;
        for (int k = 0; k < jm::OBS_MAX_SOURCES; ++k) a.source[k] = io->source[k];
        a.reset_mask = io->reset_mask; a.hist = (TIn *)io->hist; a.out = (TOut *)io->out;
        hipLaunchKernelGGL((jm::k_observe<TIn, TOut>), grid, dim3(256), 0, (hipStream_t)stream, it, dt, a, (int)(shift != 0), (long long)B);
    };
    if (dtype_in == JM_F64 && dtype_out == JM_F64) launch(double(), double());
    else if (dtype_in == JM_F64) launch(double(), float());
    else launch(float(), float());
    HIP_TRY(hipGetLastError());
    return JM_OK;
}

// ziggurat tables: computed once on the host (random.cc:66-96), one copy per device
static int32_t ziggurat_tables_on_device(jm::rnd::ZigguratTables ** out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    static std::mutex mtx;
    static std::map<int, jm::rnd::ZigguratTables *> tables;
    std::lock_guard<std::mutex> lock(mtx);
    auto it = tables.find(dev);
    if (it == tables.end())
    {
        jm::rnd::ZigguratTables host;
        jm::rnd::ziggurat_tables(host);
        jm::rnd::ZigguratTables * tab = nullptr;
        HIP_TRY(hipMalloc((void **)&tab, sizeof(host)));
        HIP_TRY(hipMemcpy(tab, &host, sizeof(host), hipMemcpyHostToDevice));
        tables[dev] = tab;
        *out = tab;
    }
    else *out = it->second;
    return JM_OK;
}

int32_t jm_block_sensor_noise(int32_t dtype, int64_t B, int32_t n_sensors, int32_t n_fields, void * data,
                              uint64_t * rng_state, const double * noise_std, const double * bias,
                              const double * rot_bias_inv, void * stream)
{
    if (!data) return fail(JM_EINVAL, "jm_block_sensor_noise: null data");
    if (B <= 0 || n_sensors <= 0 || n_fields <= 0 || n_fields > JM_NOISE_MAX_FIELDS ||
        n_sensors * n_fields > JM_NOISE_MAX_ROWS)
        return fail(JM_EINVAL, "jm_block_sensor_noise: bad sizes");
    if (dtype != JM_F64 && dtype != JM_F32) return fail(JM_EINVAL, "jm_block_sensor_noise: bad dtype");
    if (noise_std && !rng_state) return fail(JM_EINVAL, "jm_block_sensor_noise: noise needs the generator states");
    if (rot_bias_inv && (n_fields != 6 || n_sensors > JM_NOISE_MAX_ROT || !bias))
        return fail(JM_EINVAL, "jm_block_sensor_noise: the rotation bias applies to IMU fields (6 rows) with a bias");
    if (!noise_std && !bias) return JM_OK;
    jm::NoiseParams p{};
    p.n_sensors = n_sensors; p.n_fields = n_fields;
    p.has_noise = noise_std != nullptr; p.has_bias = bias != nullptr; p.has_rot = rot_bias_inv != nullptr;
    for (int i = 0; i < n_sensors * n_fields; ++i)
    {
        if (noise_std)
        {
            if (!(noise_std[i] >= 0.0)) return fail(JM_EINVAL, "jm_block_sensor_noise: negative noise standard deviation");
            p.noise_std[i] = (float)noise_std[i];
        }
        if (bias) p.bias[i] = bias[i];
    }
    if (rot_bias_inv)
        for (int s = 0; s < n_sensors; ++s)
            for (int k = 0; k < 9; ++k) p.rot[s][k] = rot_bias_inv[9 * s + k];
    jm::rnd::ZigguratTables * tab = nullptr;
    {
        const int32_t rc = ziggurat_tables_on_device(&tab);
        if (rc != JM_OK) return rc;
    }
    return launch_lanes(dtype, B, (unsigned)n_sensors, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_sensor_noise<T>), grid, dim3(256), 0, s, p, tab, (T *)data, rng_state, (long long)B);
    });
}

int32_t jm_block_sensor_delay(int32_t dtype, int64_t B, int32_t n_sensors, int32_t n_fields, void * data,
                              const void * history, const int32_t * slot, const double * times, int32_t n_history,
                              uint64_t * rng_state, const double * delay, const double * jitter, int32_t order,
                              void * stream)
{
    if (!data) return fail(JM_EINVAL, "jm_block_sensor_delay: null data");
    if (B <= 0 || n_sensors <= 0 || n_fields <= 0 || n_fields > JM_NOISE_MAX_FIELDS || n_sensors > JM_NOISE_MAX_ROWS)
        return fail(JM_EINVAL, "jm_block_sensor_delay: bad sizes");
    if (dtype != JM_F64 && dtype != JM_F32) return fail(JM_EINVAL, "jm_block_sensor_delay: bad dtype");
    if (order != 0 && order != 1)
        return fail(JM_ENOTIMPL, "`delayInterpolationOrder` must be either 0 or 1.");  // abstract_sensor.hxx:399-403
    if (history && (!slot || !times || n_history < 1 || n_history > JM_DELAY_MAX_HISTORY))
        return fail(JM_EINVAL, "jm_block_sensor_delay: the history needs 1..64 samples with their slots and times");
    if (!history && !rng_state) return JM_OK;
    jm::DelayParams p{};
    p.n_sensors = n_sensors; p.n_fields = n_fields; p.order = order;
    p.has_history = history != nullptr; p.n_hist = history ? n_history : 0;
    for (int i = 0; i < p.n_hist; ++i)
    {
        if (i > 0 && !(times[i] >= times[i - 1])) return fail(JM_EINVAL, "jm_block_sensor_delay: sample times must ascend");
        p.slot[i] = slot[i];
        p.times[i] = times[i];
    }
    for (int s = 0; s < n_sensors; ++s)
    {
        p.delay[s] = delay ? delay[s] : 0.0;
        p.jitter[s] = jitter ? (float)jitter[s] : 0.0f;
        if (!(p.delay[s] >= 0.0) || !(p.jitter[s] >= 0.0f)) return fail(JM_EINVAL, "jm_block_sensor_delay: negative delay or jitter");
    }
    return launch_lanes(dtype, B, (unsigned)n_sensors, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_sensor_delay<T>), grid, dim3(256), 0, s, p, (T *)data, (const T *)history, rng_state, (long long)B);
    });
}

int32_t jm_block_model_bias(int32_t dtype, int64_t B, int32_t njoints, int32_t first_joint, const double * nominal,
                            const float * std4, uint64_t * rng_state, const uint8_t * mask, void * model_lane, void * stream)
{
    const bool sizes_ok = B > 0 && njoints >= 1 && first_joint >= 1 && first_joint <= njoints;
    if (const int32_t rc = check_call("jm_block_model_bias", nominal && std4 && rng_state && model_lane, sizes_ok, dtype)) return rc;
    for (int i = 0; i < 4; ++i)
        if (!(std4[i] >= 0.0f)) return fail(JM_EINVAL, "jm_block_model_bias: negative standard deviation");
    jm::BiasParams p{};
    p.njoints = njoints; p.first = first_joint;
    p.inertia_std = std4[0]; p.mass_std = std4[1]; p.com_std = std4[2]; p.pos_std = std4[3];
    jm::rnd::ZigguratTables * tab = nullptr;
    const int32_t rc = ziggurat_tables_on_device(&tab);
    if (rc != JM_OK) return rc;
    return launch_lanes(dtype, B, 1, stream, [&](auto z, dim3 grid, hipStream_t s) {
        using T = decltype(z);
        hipLaunchKernelGGL((jm::k_model_bias<T>), grid, dim3(256), 0, s, p, tab, nominal, rng_state, mask, (T *)model_lane, (long long)B);
    });
}

int32_t jm_engine_rng_seed(const uint32_t * seed, int64_t B, uint64_t * state_out)
{
    if (!seed || !state_out || B <= 0) return fail(JM_EINVAL, "jm_engine_rng_seed: bad arguments");
    for (int64_t lane = 0; lane < B; ++lane)
    {
        // internal::generateState (random.hxx:20-44): two 32-bit words of the sequence, low word first
        std::seed_seq seq{seed[lane]};
        uint32_t w[2];
        seq.generate(w, w + 2);
        state_out[lane] = jm::rnd::pcg32_init((uint64_t)w[0] | ((uint64_t)w[1] << 32));
    }
    return JM_OK;
}

int32_t jm_sensor_rng_seed(const uint32_t * group_seed, int64_t B, int32_t n_sensors, uint64_t * state_out)
{
    if (!group_seed || !state_out || B <= 0 || n_sensors <= 0) return fail(JM_EINVAL, "jm_sensor_rng_seed: bad arguments");
    std::vector<uint32_t> words((size_t)n_sensors);
    for (int64_t lane = 0; lane < B; ++lane)
    {
        std::seed_seq seq{group_seed[lane]};
        seq.generate(words.begin(), words.end());
        for (int32_t s = 0; s < n_sensors; ++s) state_out[(size_t)s * B + lane] = jm::rnd::pcg32_init(words[s]);
    }
    return JM_OK;
}
}  // extern "C"
