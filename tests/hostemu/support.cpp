// Host emulation of the projected support polygon (tests only): the per-lane body of jiminy_amd/csrc/jm_support.h
// (`support_lane`: what the kernel runs) and the description check / packing of `jm_support_plan_create`, compiled by the
// host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_support.h"

namespace
{
int refuse(const std::string & why, char * error, size_t error_size)
{
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

int pack(const jm_support_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::support_pack(desc, it, dt, why)) return JM_OK;
    return refuse(why, error, error_size);
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, long long B, const jm_support_io * io, double cutoff_inner, double cutoff_outer)
{
    const jm::SupportIO<T> a{(const T *)io->pose, (const T *)io->odom_pose, (const T *)io->zmp, io->lane_mask, io->n_vertices,
                             io->vertex_index, (T *)io->vertices, (T *)io->center, (T *)io->scalars};
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane])
            jm::support_lane<T>(it.data(), a, (T)cutoff_inner, (T)cutoff_outer, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_support_pack(const jm_support_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_support(const jm_support_desc * desc, int dtype, long long B, const jm_support_io * io, double cutoff_inner,
                           double cutoff_outer, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    std::string why;
    if (!jm::support_cutoffs_check(cutoff_inner, cutoff_outer, why)) return refuse(why, error, error_size);
    if (dtype == JM_F64) all_lanes<double>(it, B, io, cutoff_inner, cutoff_outer);
    else all_lanes<float>(it, B, io, cutoff_inner, cutoff_outer);
    return JM_OK;
}
