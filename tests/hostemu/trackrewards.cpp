// Host emulation of the tracking rewards block (tests only): the per-lane body of jiminy_amd/csrc/jm_trackrewards.h
// (`trackrewards_lane`: what the kernel runs) and the description check / packing of `jm_trackrewards_plan_create`, compiled by
// the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_trackrewards.h"

namespace
{
int pack(const jm_trackrewards_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::trackrewards_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T> void all_lanes(const std::vector<int32_t> & it, long long B, const jm_trackrewards_io * io, const double * cutoff)
{
    const jm::TrkRewIO<T> a{(const T *)io->pose, (const T *)io->pose_reference, (const T *)io->v_avg, (const T *)io->quat_no_yaw,
                            (const T *)io->v_avg_reference, (const T *)io->quat_no_yaw_reference, (const T *)io->dcm,
                            (const T *)io->dcm_reference, (const T *)io->position, (const T *)io->position_reference, io->lane_mask,
                            (T *)io->value, (T *)io->reference, (T *)io->rewards};
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane]) jm::trackrewards_lane<T>(it.data(), a, cutoff, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_trackrewards_pack(const jm_trackrewards_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

// the argument checks of `jm_block_tracking_rewards` and its treatment of the cutoffs, then every lane of the mask
extern "C" int emu_tracking_rewards(const jm_trackrewards_desc * desc, int dtype, long long B, const jm_trackrewards_io * io,
                                    const double * cutoff, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || !cutoff || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    double c[jm::TR_TERMS];
    for (int k = 0; k < jm::TR_TERMS; ++k) c[k] = cutoff[k] > 0.0 ? cutoff[k] : 0.0;
    if (dtype == JM_F64) all_lanes<double>(it, B, io, c);
    else all_lanes<float>(it, B, io, c);
    return JM_OK;
}
