// Host emulation of the reference trajectories block (tests only): the per-lane body of jiminy_amd/csrc/jm_trajectory.h
// (`trajectory_state_lane`: what the kernel runs) and the description check / packing of `jm_trajectory_plan_create`, compiled
// by the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_trajectory.h"

namespace
{
int pack(const jm_trajectory_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::trajectory_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, const std::vector<double> & dt, const void * data, long long B, const jm_trajectory_io * io)
{
    const jm::TrajIO<T> a{io->time, io->trajectory, io->time_offset, io->lane_mask, (T *)io->q, (T *)io->v, (T *)io->a,
                          (T *)io->command, (T *)io->odom_pose, (T *)io->position, io->status};
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane]) jm::trajectory_state_lane<T>(it.data(), dt.data(), (const T *)data, a, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_trajectory_pack(const jm_trajectory_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_trajectory(const jm_trajectory_desc * desc, int dtype, long long B, const jm_trajectory_io * io, char * error,
                              size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || !io->time || !io->trajectory || !io->time_offset || B <= 0 || dtype != desc->dtype) return JM_EINVAL;
    if (dtype == JM_F64) all_lanes<double>(it, dt, desc->data, B, io);
    else all_lanes<float>(it, dt, desc->data, B, io);
    return JM_OK;
}
