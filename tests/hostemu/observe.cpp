// Host emulation of the observation assembly (tests only): the per-(element, lane) body of jiminy_amd/csrc/jm_observe.h
// (`observe_frame`: what the kernel runs), the description check / packing of `jm_observe_plan_create` and the dtype and
// aliasing checks of `jm_block_observe`, compiled by the host compiler and run pair after pair.
#define JM_HOST_EMU 1
#include <cstring>

#include "../../jiminy_amd/csrc/jm_observe.h"

namespace
{
int refuse(const std::string & why, char * error, size_t error_size)
{
    if (error && error_size) { std::strncpy(error, why.c_str(), error_size - 1); error[error_size - 1] = 0; }
    return JM_EINVAL;
}

template<class TIn, class TOut>
void all_pairs(const std::vector<int32_t> & it, const std::vector<double> & dt, long long B, const jm_observe_io * io, bool shift)
{
    jm::ObserveIO<TIn, TOut> a;
    for (int k = 0; k < jm::OBS_MAX_SOURCES; ++k) a.source[k] = io->source[k];
    a.reset_mask = io->reset_mask; a.hist = (TIn *)io->hist; a.out = (TOut *)io->out;
    const int D = it[1], S = it[2], W = it[3];
    const int32_t * pos = it.data() + jm::obs_it_pos(D);
    for (int e = 0; e < D; ++e)
        for (long long lane = 0; lane < B; ++lane)
        {
            const bool reset = a.reset_mask && a.reset_mask[lane] != 0;
            for (int s = 0; s < S; ++s)
            {
                const TIn x = jm::observe_frame<TIn, TOut>(it.data(), dt.data(), a, D, S, e, s, shift, reset, B, lane);
                const int p = pos[(long long)s * D + e];
                if (p >= 0) a.out[lane * W + p] = (TOut)x;
            }
        }
}
}  // namespace

// the description check alone
extern "C" int emu_observe_pack(const jm_observe_desc * desc, char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    std::string why;
    return jm::observe_pack(desc, it, dt, why) ? JM_OK : refuse(why, error, error_size);
}

extern "C" int emu_observe(const jm_observe_desc * desc, int dtype_in, int dtype_out, long long B, const jm_observe_io * io, int shift,
                           char * error, size_t error_size)
{
    std::vector<int32_t> it;
    std::vector<double> dt;
    std::string why;
    if (!jm::observe_pack(desc, it, dt, why)) return refuse(why, error, error_size);
    if (!io || B <= 0) return refuse("jm_block_observe: bad sizes", error, error_size);
    if (!jm::observe_dtype_check(dtype_in, dtype_out, why)) return refuse(why, error, error_size);
    if (!jm::observe_alias_check(it, io, B, dtype_in == JM_F64 ? 8 : 4, dtype_out == JM_F64 ? 8 : 4, why)) return refuse(why, error, error_size);
    if (dtype_in == JM_F64 && dtype_out == JM_F64) all_pairs<double, double>(it, dt, B, io, shift != 0);
    else if (dtype_in == JM_F64) all_pairs<double, float>(it, dt, B, io, shift != 0);
    else all_pairs<float, float>(it, dt, B, io, shift != 0);
    return JM_OK;
}

// the sizes of the structures of the header, for the ctypes mirrors
extern "C" void emu_observe_sizes(int * out)
{
    out[0] = (int)sizeof(jm_observe_desc);
    out[1] = (int)sizeof(jm_observe_io);
}
