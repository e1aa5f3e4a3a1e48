// Host emulation of the attitude observers (tests only): the per-lane bodies of jiminy_amd/csrc/jm_attitude.h
// (`attitude_init_lane`, `mahony_observer_lane`, `body_observer_lane`, `mahony_lane` with one pair of gains: what the four
// kernels run) and the description check / packing of `jm_attitude_plan_create`, compiled by the host compiler and run lane
// after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_attitude.h"

namespace
{
int pack(const jm_attitude_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::attitude_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void init_all(const std::vector<int32_t> & it, const std::vector<double> & dt, int n_imu, long long B, const void * q, const void * imu,
              const uint8_t * mask, int exact_init, void * quat, void * omega, void * cf, void * bias, void * twist, void * rpy)
{
    for (long long lane = 0; lane < B; ++lane)
        if (!mask || mask[lane])
            jm::attitude_init_lane<T>(it.data(), dt.data(), n_imu, exact_init, (const T *)q, (const T *)imu, (T *)quat, (T *)omega,
                                      (T *)cf, (T *)bias, (T *)twist, (T *)rpy, B, lane);
}
}  // namespace

extern "C" int emu_attitude_init(const jm_attitude_desc * desc, int dtype, long long B, const void * q, const void * imu,
                                 const uint8_t * mask, int exact_init, void * quat, void * omega, void * cf, void * bias, void * twist,
                                 void * rpy, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!q || !imu || !quat || !omega || !cf || !bias || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (dtype == JM_F64) init_all<double>(it, dt, desc->n_imu, B, q, imu, mask, exact_init, quat, omega, cf, bias, twist, rpy);
    else init_all<float>(it, dt, desc->n_imu, B, q, imu, mask, exact_init, quat, omega, cf, bias, twist, rpy);
    return JM_OK;
}

extern "C" int emu_mahony_observer(const jm_attitude_desc * desc, int dtype, long long B, const void * imu, void * quat, void * omega,
                                   void * cf, void * bias, double step, int ignore_twist, void * rpy, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!imu || !quat || !omega || !cf || !bias || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    for (long long lane = 0; lane < B; ++lane)
    {
        if (dtype == JM_F64)
            jm::mahony_observer_lane<double>(dt.data(), desc->n_imu, (const double *)imu, (double *)quat, (double *)omega, (double *)cf,
                                             (double *)bias, step, ignore_twist, (double *)rpy, B, lane);
        else
            jm::mahony_observer_lane<float>(dt.data(), desc->n_imu, (const float *)imu, (float *)quat, (float *)omega, (float *)cf,
                                            (float *)bias, (float)step, ignore_twist, (float *)rpy, B, lane);
    }
    return JM_OK;
}

extern "C" int emu_body_observer(const jm_attitude_desc * desc, int dtype, long long B, const void * imu_quat, const void * imu_omega,
                                 void * quat, void * omega, void * twist, int twist_mode, double time_constant_inv, double step,
                                 void * rpy, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!imu_quat || !imu_omega || !quat || !omega || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (twist_mode < 0 || twist_mode > 2 || (twist_mode == 2 && !twist)) return JM_EINVAL;
    for (long long lane = 0; lane < B; ++lane)
    {
        if (dtype == JM_F64)
            jm::body_observer_lane<double>(dt.data(), desc->n_imu, (const double *)imu_quat, (const double *)imu_omega, (double *)quat,
                                           (double *)omega, (double *)twist, twist_mode, time_constant_inv, step, (double *)rpy, B, lane);
        else
            jm::body_observer_lane<float>(dt.data(), desc->n_imu, (const float *)imu_quat, (const float *)imu_omega, (float *)quat,
                                          (float *)omega, (float *)twist, twist_mode, time_constant_inv, step, (float *)rpy, B, lane);
    }
    return JM_OK;
}

// the plain `mahony_filter` function (`k_mahony`: one pair of gains for every IMU, no plan)
extern "C" int emu_mahony_filter(int dtype, long long B, int n_imu, const void * imu, void * quat, void * omega, void * cf, void * bias,
                                 double kp, double ki, double step)
{
    if (!imu || !quat || !omega || !cf || !bias || B <= 0 || n_imu <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    for (long long lane = 0; lane < B; ++lane)
    {
        if (dtype == JM_F64)
            jm::mahony_lane<jm::TILT_FUSED>(n_imu, jm::UniformGains<double>{kp, ki}, (const double *)imu, (double *)quat, (double *)omega,
                                            (double *)cf, (double *)bias, step, B, lane);
        else
            jm::mahony_lane<jm::TILT_FUSED>(n_imu, jm::UniformGains<float>{(float)kp, (float)ki}, (const float *)imu, (float *)quat,
                                            (float *)omega, (float *)cf, (float *)bias, (float)step, B, lane);
    }
    return JM_OK;
}
