// Host emulation of the DeformationEstimator block (tests only): the per-lane body of jiminy_amd/csrc/jm_deform.h
// (`deform_lane`, what `k_deformation_estimator` runs) and the description check / packing of `jm_deform_plan_create`,
// compiled by the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_deform.h"

extern "C" int emu_deformation_estimator(const jm_deform_desc * desc, int dtype, long long B, const void * encoder,
                                         const void * imu_quat, void * out_quat, void * out_rpy, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    std::string why;
    if (!jm::deform_pack(desc, it, dt, why))
    {
        if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
        return JM_EINVAL;
    }
    if (!encoder || !imu_quat || !out_quat || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    for (long long lane = 0; lane < B; ++lane)
    {
        if (dtype == JM_F64)
            jm::deform_lane<double>(it.data(), dt.data(), desc->n_imu, desc->n_flex, desc->ignore_twist, (const double *)encoder,
                                    (const double *)imu_quat, (double *)out_quat, (double *)out_rpy, B, lane);
        else
            jm::deform_lane<float>(it.data(), dt.data(), desc->n_imu, desc->n_flex, desc->ignore_twist, (const float *)encoder,
                                   (const float *)imu_quat, (float *)out_quat, (float *)out_rpy, B, lane);
    }
    return JM_OK;
}
