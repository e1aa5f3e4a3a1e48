// Host emulation of the frame kinematics block (tests only): the per-lane bodies of jiminy_amd/csrc/jm_frames.h
// (`frame_kinematics_lane`, `frame_average_lane`: what the two kernels run) and the description check / packing of
// `jm_frames_plan_create`, compiled by the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_frames.h"

namespace
{
int pack(const jm_frames_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::frames_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void kinematics_all(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const void * q, const void * v,
                    const void * model_lane, const uint8_t * mask, void * pose, void * pose_prev, void * rpy, void * vel)
{
    for (long long lane = 0; lane < B; ++lane)
        if (!mask || mask[lane])
            jm::frame_kinematics_lane<T>(it.data(), dt.data(), (const T *)q, (const T *)v, (const T *)model_lane, (T *)pose,
                                         (T *)pose_prev, (T *)rpy, (T *)vel, B, lane);
}

template<class T>
void average_all(const std::vector<int32_t> & it, long long B, void * pose_prev, const void * pose, double inv_step_dt, void * v_avg,
                 void * pose_mean, void * quat_no_yaw)
{
    for (long long lane = 0; lane < B; ++lane)
        jm::frame_average_lane<T>(it.data(), (T *)pose_prev, (const T *)pose, (T)inv_step_dt, (T *)v_avg, (T *)pose_mean,
                                  (T *)quat_no_yaw, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_frames_pack(const jm_frames_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_frame_kinematics(const jm_frames_desc * desc, int dtype, long long B, const void * q, const void * v,
                                    const void * model_lane, const uint8_t * mask, void * pose, void * pose_prev, void * rpy,
                                    void * vel, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!q || (vel && !v) || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (dtype == JM_F64) kinematics_all<double>(it, dt, B, q, v, model_lane, mask, pose, pose_prev, rpy, vel);
    else kinematics_all<float>(it, dt, B, q, v, model_lane, mask, pose, pose_prev, rpy, vel);
    return JM_OK;
}

extern "C" int emu_frame_average(const jm_frames_desc * desc, int dtype, long long B, void * pose_prev, const void * pose,
                                 double inv_step_dt, void * v_avg, void * pose_mean, void * quat_no_yaw, char * error,
                                 size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!pose_prev || !pose || pose_prev == pose || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (dtype == JM_F64) average_all<double>(it, B, pose_prev, pose, inv_step_dt, v_avg, pose_mean, quat_no_yaw);
    else average_all<float>(it, B, pose_prev, pose, inv_step_dt, v_avg, pose_mean, quat_no_yaw);
    return JM_OK;
}
