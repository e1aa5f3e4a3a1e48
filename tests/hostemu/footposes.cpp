// Host emulation of the foot pose quantities (tests only): the per-lane body of jiminy_amd/csrc/jm_footposes.h
// (`footposes_lane`: what the kernel runs) and the description check / packing of `jm_footposes_plan_create`, compiled by
// the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_footposes.h"

namespace
{
int pack(const jm_footposes_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::footposes_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const jm_footposes_io * io,
               double position_cutoff, double orientation_cutoff)
{
    const jm::FootIO<T> a{(const T *)io->pose, (const T *)io->reference_relative_pose, io->lane_mask, (T *)io->mean_pose,
                          (T *)io->mean_odom_pose, (T *)io->relative_pose, (T *)io->tracking_error, (T *)io->scalars};
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane])
            jm::footposes_lane<T>(it.data(), dt.data(), a, (T)position_cutoff, (T)orientation_cutoff, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_footposes_pack(const jm_footposes_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_footposes(const jm_footposes_desc * desc, int dtype, long long B, const jm_footposes_io * io,
                             double position_cutoff, double orientation_cutoff, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (dtype == JM_F64) all_lanes<double>(it, dt, B, io, position_cutoff, orientation_cutoff);
    else all_lanes<float>(it, dt, B, io, position_cutoff, orientation_cutoff);
    return JM_OK;
}
