// Host emulation of the locomotion quantities on height-map ground (tests only): `locomotion_lane<T, true>` of
// jiminy_amd/csrc/jm_locomotion.h (what `jm_block_locomotion_ground` runs) and the check of its ground description,
// compiled by the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_locomotion.h"

namespace
{
int failed(const std::string & why, char * error, size_t error_size)
{
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const jm_locomotion_io * io,
               const jm_locomotion_ground * g, double momentum_cutoff, double friction_cutoff)
{
    jm::LocoIO<T> a{(const T *)io->centroidal, (const T *)io->q_root, (const T *)io->model_lane, (const T *)io->con_lambda,
                    io->con_flags, (const T *)io->v_avg, (const T *)io->quat_no_yaw, (const T *)io->pose, io->lane_mask,
                    (T *)io->com, (T *)io->vcom, (T *)io->odom_pose, (T *)io->zmp, (T *)io->dcm, (T *)io->h_angular,
                    (T *)io->contact_force_rel, (T *)io->foot_force_vertical, (T *)io->scalars};
    if (g)
    {
        a.contact_ground = (T *)g->contact_ground;
        if (g->heights)
        {
            a.ground_h = (const T *)g->heights; a.ground_nx = g->nx; a.ground_ny = g->ny;
            a.ground_x0 = (T)g->x0; a.ground_y0 = (T)g->y0; a.ground_dx = (T)g->dx; a.ground_dy = (T)g->dy;
            a.ground_off = (const T *)g->offsets;
        }
    }
    for (long long lane = 0; lane < B; ++lane)
        if (!a.lane_mask || a.lane_mask[lane])
            jm::locomotion_lane<T, true>(it.data(), dt.data(), a, (T)momentum_cutoff, (T)friction_cutoff, B, lane);
}
}  // namespace

extern "C" int emu_locomotion_ground(const jm_locomotion_desc * desc, int dtype, long long B, const jm_locomotion_io * io,
                                     const jm_locomotion_ground * ground, double momentum_cutoff, double friction_cutoff,
                                     char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    std::string why;
    if (!jm::locomotion_pack(desc, it, dt, why)) return failed(why, error, error_size);
    if (!io || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (!jm::locomotion_ground_check(ground, io, why)) return failed(why, error, error_size);
    if (dtype == JM_F64) all_lanes<double>(it, dt, B, io, ground, momentum_cutoff, friction_cutoff);
    else all_lanes<float>(it, dt, B, io, ground, momentum_cutoff, friction_cutoff);
    return JM_OK;
}
