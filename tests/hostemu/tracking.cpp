// Host emulation of the tracking windows (tests only): the per-lane body of jiminy_amd/csrc/jm_tracking.h (`tracking_lane`:
// what the kernel runs) and the description check / packing of `jm_tracking_plan_create`, compiled by the host compiler and
// run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_tracking.h"

namespace
{
int pack(const jm_tracking_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::tracking_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T> void all_lanes(const std::vector<int32_t> & it, long long B, const jm_tracking_io * io, int mode, double odometry_cutoff)
{
    const jm::TrkIO<T> a{(const T *)io->odom_pose, (const T *)io->reference_odom_pose, (const T *)io->relative_pose,
                         (const T *)io->reference_relative_pose, (const T *)io->position, (const T *)io->reference_position,
                         io->lane_mask, io->count, (T *)io->odom_ring, (T *)io->yaw_prev, (T *)io->yaw_ring, (T *)io->foot_ring,
                         (T *)io->motor_ring, (T *)io->delta_odom, (T *)io->delta_odom_reference, (T *)io->scalars};
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane]) jm::tracking_lane<T>(it.data(), a, mode, (T)odometry_cutoff, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_tracking_pack(const jm_tracking_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_tracking(const jm_tracking_desc * desc, int dtype, long long B, const jm_tracking_io * io, int mode,
                            double odometry_cutoff, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || B <= 0 || (dtype != JM_F64 && dtype != JM_F32) || (mode != jm::TRK_RESTART && mode != jm::TRK_PUSH)) return JM_EINVAL;
    if (dtype == JM_F64) all_lanes<double>(it, B, io, mode, odometry_cutoff);
    else all_lanes<float>(it, B, io, mode, odometry_cutoff);
    return JM_OK;
}
