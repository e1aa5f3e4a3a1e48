// Host emulation of the locomotion quantities (tests only): the per-lane body of jiminy_amd/csrc/jm_locomotion.h
// (`locomotion_lane`: what the kernel runs) and the description check / packing of `jm_locomotion_plan_create`, compiled by
// the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_locomotion.h"

namespace
{
int pack(const jm_locomotion_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::locomotion_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const jm_locomotion_io * io,
               double momentum_cutoff, double friction_cutoff)
{
    const jm::LocoIO<T> a{(const T *)io->centroidal, (const T *)io->q_root, (const T *)io->model_lane, (const T *)io->con_lambda,
                          io->con_flags, (const T *)io->v_avg, (const T *)io->quat_no_yaw, (const T *)io->pose, io->lane_mask,
                          (T *)io->com, (T *)io->vcom, (T *)io->odom_pose, (T *)io->zmp, (T *)io->dcm, (T *)io->h_angular,
                          (T *)io->contact_force_rel, (T *)io->foot_force_vertical, (T *)io->scalars};
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane])
            jm::locomotion_lane<T>(it.data(), dt.data(), a, (T)momentum_cutoff, (T)friction_cutoff, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_locomotion_pack(const jm_locomotion_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

extern "C" int emu_locomotion(const jm_locomotion_desc * desc, int dtype, long long B, const jm_locomotion_io * io,
                              double momentum_cutoff, double friction_cutoff, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!io || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (dtype == JM_F64) all_lanes<double>(it, dt, B, io, momentum_cutoff, friction_cutoff);
    else all_lanes<float>(it, dt, B, io, momentum_cutoff, friction_cutoff);
    return JM_OK;
}
