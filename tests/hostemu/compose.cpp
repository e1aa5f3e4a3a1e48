// Host emulation of the composition layer (tests only): the per-lane body of jiminy_amd/csrc/jm_compose.h (`compose_lane`:
// what the kernel runs) and the description check / packing of `jm_compose_plan_create`, compiled by the host compiler and
// run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_compose.h"

namespace
{
int refuse(const std::string & why, char * error, size_t error_size)
{
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

int pack(const jm_compose_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::compose_pack(desc, it, dt, why)) return JM_OK;
    return refuse(why, error, error_size);
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const jm_compose_io * io, bool training)
{
    jm::ComposeIO<T> a;
    for (int k = 0; k < jm::CMP_MAX_SOURCES; ++k) a.source[k] = io->source[k];
    a.time = (const T *)io->time; a.base_terminated = io->base_terminated; a.base_truncated = io->base_truncated;
    a.lane_mask = io->lane_mask; a.reward = (T *)io->reward; a.node_value = (T *)io->node_value;
    a.terminated = io->terminated; a.truncated = io->truncated; a.trigger = io->trigger; a.violations = io->violations;
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane])
            jm::compose_lane<T>(it.data(), dt.data(), a, training, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_compose_pack(const jm_compose_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_compose(const jm_compose_desc * desc, int dtype, long long B, const jm_compose_io * io, int training, char * error,
                           size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (dtype == JM_F64) all_lanes<double>(it, dt, B, io, training != 0);
    else all_lanes<float>(it, dt, B, io, training != 0);
    return JM_OK;
}
