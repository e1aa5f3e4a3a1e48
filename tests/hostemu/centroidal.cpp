// Host emulation of the centroidal state block (tests only): the per-lane body of jiminy_amd/csrc/jm_centroidal.h
// (`centroidal_lane`: what the kernel runs) and the description check / packing of `jm_centroidal_plan_create`, compiled by
// the host compiler and run lane after lane.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_centroidal.h"

namespace
{
int pack(const jm_centroidal_desc * desc, std::vector<int32_t> & it, std::vector<double> & dt, char * error, size_t error_size)
{
    std::string why;
    if (jm::centroidal_pack(desc, it, dt, why)) return JM_OK;
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class T>
void all_lanes(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const void * q, const void * v,
               const void * a, const uint8_t * mask, void * out)
{
    for (long long lane = 0; lane < B; ++lane)
        if (!mask || mask[lane])
            jm::centroidal_lane<T>(it.data(), dt.data(), (const T *)q, (const T *)v, (const T *)a, (T *)out, B, lane);
}
}  // namespace

// the description check alone
extern "C" int emu_centroidal_pack(const jm_centroidal_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    return pack(desc, it, dt, error, error_size);
}

// the argument checks of `jm_block_centroidal_state`, then every lane of the mask
extern "C" int emu_centroidal_state(const jm_centroidal_desc * desc, int dtype, long long B, const void * q, const void * v,
                                    const void * a, const uint8_t * mask, void * centroidal, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    if (pack(desc, it, dt, error, error_size) != JM_OK) return JM_EINVAL;
    if (!q || !v || B <= 0 || (dtype != JM_F64 && dtype != JM_F32)) return JM_EINVAL;
    if (!centroidal) return JM_OK;
    if (dtype == JM_F64) all_lanes<double>(it, dt, B, q, v, a, mask, centroidal);
    else all_lanes<float>(it, dt, B, q, v, a, mask, centroidal);
    return JM_OK;
}
