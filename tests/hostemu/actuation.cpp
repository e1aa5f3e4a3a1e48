// Host emulation of the actuated-joint quantities (tests only): the per-lane body of jiminy_amd/csrc/jm_actuation.h
// (`actuation_lane`: what the kernel runs) and the description check / packing of `jm_actuation_plan_create`, compiled by
// the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_actuation.h"

namespace
{
int pack(const jm_actuation_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::actuation_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const jm_actuation_io * io, int mode,
               int motor_side, double position_margin, double velocity_max, double power_cutoff)
{
    const jm::ActIO<T> a{(const T *)io->q, (const T *)io->v, (const T *)io->a, (const T *)io->command, io->lane_mask,
                         (T *)io->position, (T *)io->velocity, (T *)io->acceleration, (T *)io->bound_low, (T *)io->bound_high,
                         io->safety, (T *)io->scalars, (T *)io->power_ring, io->power_count};
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane])
            jm::actuation_lane<T>(it.data(), dt.data(), a, mode, motor_side != 0, (T)position_margin, (T)velocity_max, (T)power_cutoff, B,
                                  lane);
}
}  // namespace

// the description check alone
extern "C" int emu_actuation_pack(const jm_actuation_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_actuation(const jm_actuation_desc * desc, int dtype, long long B, const jm_actuation_io * io, int mode, int motor_side,
                             double position_margin, double velocity_max, double power_cutoff, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || B <= 0 || (dtype != JM_F64 && dtype != JM_F32) || (mode != jm::ACT_RESTART && mode != jm::ACT_PUSH)) return JM_EINVAL;
    if (dtype == JM_F64) all_lanes<double>(it, dt, B, io, mode, motor_side, position_margin, velocity_max, power_cutoff);
    else all_lanes<float>(it, dt, B, io, mode, motor_side, position_margin, velocity_max, power_cutoff);
    return JM_OK;
}
