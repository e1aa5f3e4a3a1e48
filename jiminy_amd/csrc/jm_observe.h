// jm_observe.h -- the observation side of the reference's gym pipelines as one batched HIP kernel: what
// `FlattenObservation(StackObservation(NormalizeObservation(ScaleObservation(AdaptLayoutObservation(env)))))` hands to the
// learner, assembled from the rows other blocks left on the device.  Every source is `[rows][B]` (lane-minor) like the physics
// state; the result is `out [B][W]` (lane-major), so the kernel is a gather, a short chain of rounded operations, a rolling
// history and a transpose.  It depends on no topology: what it reads is a table of base pointers handed over at launch and a
// packed plan.
//
// Reference (python/gym_jiminy/common/gym_jiminy/common/wrappers):
//   _adapt_layout, AdaptLayoutObservation, FilterObservation      observation_layout.py:36-311, :314-443, :446-540
//   _array_scale, ScaleObservation                                scale.py:31-39, :141-244
//   NormalizeObservation                                          normalize.py:49-114
//   StackObservation                                              observation_stack.py:40-265
//   FlattenObservation                                            flatten.py
//
// One *element* is one scalar of one kept leaf: a (slot, row), at most 4 multipliers applied one after the other (each product
// rounded on its own: `ScaleObservation` multiplies by `1.0 / scale` once per operation), then `(x - mean) / scale`.  One
// *position* is one column of `out`: an element and its age (0: the current frame).  The history `hist [num_stack][D][B]` is
// shifted physically: frame s takes frame s + 1 and the newest frame takes the current value, by the one thread that owns the
// (element, lane) pair through the whole stack, so that no ring counter and no host state exist.
#pragma once
#include "jm_frames.h"

namespace jm
{
constexpr int OBS_MAX_SOURCES = 16, OBS_MAX_ELEMENTS = 2048, OBS_MAX_STACK = 16, OBS_MAX_POSITIONS = 8192, OBS_MAX_MULTIPLIERS = 4;
constexpr int OBS_TILE = 64;      // elements x lanes of one block
// ---- the packed plan.  `it`: [n_sources, D, num_stack, W, 0, 0, 0, 0 | rows of the 16 sources | 3 ints of each of the D elements:
// slot, row, is stacked | the position of every (frame, element), `[num_stack][D]`, frame num_stack - 1 being the current one;
// -1: not emitted].  `dt`: [the 4 multipliers of the D elements | mean of the D elements | scale of the D elements].
constexpr int OBS_IT_SRC_ROWS = 8, OBS_IT_ELEM = OBS_IT_SRC_ROWS + OBS_MAX_SOURCES, OBS_ELEM_INTS = 3;
constexpr int obs_it_pos(int D) { return OBS_IT_ELEM + OBS_ELEM_INTS * D; }

inline bool observe_pack(const jm_observe_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_observe_plan_create: ";
    const auto no = [&](const std::string & what) { why = who + what; return false; };
    const auto at = [](const char * what, int i) { return std::string(what) + " " + std::to_string(i); };
    if (!d) return no("null description");
    if (d->n_sources < 1 || d->n_sources > OBS_MAX_SOURCES) return no("1 to 16 sources are supported, got " + std::to_string(d->n_sources));
    if (d->n_elements < 1) return no("The resulting observation space must not be empty.");      // (observation_layout.py:413-415)
    if (d->n_elements > OBS_MAX_ELEMENTS) return no("at most 2048 elements are supported, got " + std::to_string(d->n_elements));
    if (d->num_stack < 1 || d->num_stack > OBS_MAX_STACK) return no("num_stack must be in [1, 16], got " + std::to_string(d->num_stack));
    if (d->n_positions < 1 || d->n_positions > OBS_MAX_POSITIONS)
        return no("1 to 8192 output positions are supported, got " + std::to_string(d->n_positions));
    if (d->n_multipliers < 0) return no("bad sizes: the number of multipliers");
    if (!d->source_rows || !d->elem_slot || !d->elem_row || !d->elem_mult_start || !d->elem_mult_count || !d->elem_mean || !d->elem_scale ||
        (d->n_multipliers > 0 && !d->multiplier) || !d->pos_elem || !d->pos_age)
        return no("null array in the description");
    const int D = d->n_elements, S = d->num_stack, W = d->n_positions;
    it.assign((size_t)obs_it_pos(D) + (size_t)S * D, -1);
    dt.assign((size_t)(OBS_MAX_MULTIPLIERS + 2) * D, 1.0);
    for (int k = 0; k < OBS_IT_ELEM; ++k) it[k] = 0;
    it[0] = d->n_sources; it[1] = D; it[2] = S; it[3] = W;
    for (int s = 0; s < d->n_sources; ++s)
    {
        if (d->source_rows[s] < 1) return no(at("source", s) + " has no rows");
        it[OBS_IT_SRC_ROWS + s] = d->source_rows[s];
    }
    for (int e = 0; e < D; ++e)
    {
        const int slot = d->elem_slot[e], row = d->elem_row[e], start = d->elem_mult_start[e], count = d->elem_mult_count[e];
        if (slot < 0 || slot >= d->n_sources)
            return no(at("element", e) + " reads slot " + std::to_string(slot) + ", out of range [0, " + std::to_string(d->n_sources) + ")");
        if (row < 0 || row >= d->source_rows[slot])
            return no(at("element", e) + " reads row " + std::to_string(row) + ", out of range [0, " + std::to_string(d->source_rows[slot]) +
                      ") of its slot");
        if (count < 0 || count > OBS_MAX_MULTIPLIERS)
            return no(at("element", e) + " has " + std::to_string(count) + " multipliers, at most 4 per element are supported");
        if (count > 0 && (start < 0 || start > d->n_multipliers - count)) return no(at("element", e) + " has multipliers out of range");
        int32_t * elem = &it[OBS_IT_ELEM + OBS_ELEM_INTS * e];
        elem[0] = slot; elem[1] = row; elem[2] = 0;
        for (int m = 0; m < count; ++m)
        {
            const double f = d->multiplier[start + m];
            if (f != f) return no(at("element", e) + " has a multiplier that is not a number");
            dt[(size_t)OBS_MAX_MULTIPLIERS * e + m] = f;
        }
        const double mean = d->elem_mean[e], scale = d->elem_scale[e];
        if (mean != mean || scale != scale) return no(at("element", e) + " has a mean or a scale that is not a number");
        if (scale == 0.0) return no(at("element", e) + " has a zero scale");
        dt[(size_t)OBS_MAX_MULTIPLIERS * D + e] = mean;
        dt[(size_t)(OBS_MAX_MULTIPLIERS + 1) * D + e] = scale;
    }
    // the positions: an element is emitted once (age 0, not stacked) or at every age (stacked)
    std::vector<int> count((size_t)D, 0);
    for (int p = 0; p < W; ++p)
    {
        const int e = d->pos_elem[p], age = d->pos_age[p];
        if (e < 0 || e >= D) return no(at("position", p) + " holds element " + std::to_string(e) + ", out of range [0, " + std::to_string(D) + ")");
        if (age < 0 || age >= S) return no(at("position", p) + " has age " + std::to_string(age) + ", out of range [0, " + std::to_string(S) + ")");
        int32_t & cell = it[(size_t)obs_it_pos(D) + (size_t)(S - 1 - age) * D + e];
        if (cell >= 0) return no(at("position", p) + " repeats position " + std::to_string(cell) + ": an element is emitted once per age");
        cell = p;
        ++count[e];
    }
    for (int e = 0; e < D; ++e)
    {
        const bool current = it[(size_t)obs_it_pos(D) + (size_t)(S - 1) * D + e] >= 0;
        if (!current || (count[e] != 1 && count[e] != S))
            return no(at("element", e) + " is emitted at " + std::to_string(count[e]) + " ages: once (age 0) or at every age of the stack");
        it[OBS_IT_ELEM + OBS_ELEM_INTS * e + 2] = S > 1 && count[e] == S;
    }
    return true;
}

// the pairs of scalar types the kernel is built for: the cast to the output type is the last operation and never widens
inline bool observe_dtype_check(int32_t dtype_in, int32_t dtype_out, std::string & why)
{
    if ((dtype_in != JM_F64 && dtype_in != JM_F32) || (dtype_out != JM_F64 && dtype_out != JM_F32))
    { why = "jm_block_observe: bad dtype"; return false; }
    if (dtype_in == JM_F32 && dtype_out == JM_F64)
    { why = "jm_block_observe: float32 sources with a float64 output are not supported (float64 -> float64, float64 -> float32, float32 -> float32)"; return false; }
    return true;
}

// `out` may alias neither a source nor the history: the transposed writes of one block would land in what another still reads
inline bool observe_alias_check(const std::vector<int32_t> & it, const jm_observe_io * io, long long B, size_t size_in, size_t size_out,
                                std::string & why)
{
    const auto overlap = [](const void * a, size_t na, const void * b, size_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + nb && y < x + na;
    };
    const int n_sources = it[0], D = it[1], S = it[2], W = it[3];
    const size_t n_out = (size_t)B * W * size_out;
    if (!io->out || !io->hist) { why = "jm_block_observe: null argument"; return false; }
    if (overlap(io->out, n_out, io->hist, (size_t)S * D * B * size_in)) { why = "jm_block_observe: out aliases the history"; return false; }
    for (int s = 0; s < n_sources; ++s)
    {
        if (!io->source[s]) { why = "jm_block_observe: source " + std::to_string(s) + " is null"; return false; }
        if (overlap(io->out, n_out, io->source[s], (size_t)it[OBS_IT_SRC_ROWS + s] * B * size_in))
        { why = "jm_block_observe: out aliases source " + std::to_string(s); return false; }
    }
    return true;
}

template<class TIn, class TOut> struct ObserveIO
{
    const void * source[OBS_MAX_SOURCES];   // base pointer of every slot, `[rows][B]` of TIn
    const uint8_t * reset_mask;             // [B] lanes whose older frames restart from zero (NULL: none)
    TIn * hist;                             // [num_stack][D][B]
    TOut * out;                             // [B][W]
};

// the current value of element `e` on one lane.  Only IEEE basic operations, each rounded on its own: the chain has a fixed
// length of 4 (multiplying by 1.0 is exact) and the last product does not contract into the subtraction.
template<class TIn, class TOut>
JM_DEV TIn observe_value(const int32_t * __restrict__ it, const double * __restrict__ dt, const ObserveIO<TIn, TOut> & io, int D, int e,
                         long long B, long long lane)
{
    const int32_t * elem = it + OBS_IT_ELEM + OBS_ELEM_INTS * e;
    const int slot = elem[0];
    const void * base = io.source[0];
#pragma unroll
    for (int k = 1; k < OBS_MAX_SOURCES; ++k) base = slot == k ? io.source[k] : base;
    TIn x = ((const TIn *)base)[(long long)elem[1] * B + lane];
#pragma unroll
    for (int m = 0; m < OBS_MAX_MULTIPLIERS; ++m) x = frame_product(x * (TIn)dt[OBS_MAX_MULTIPLIERS * e + m]);
    return (x - (TIn)dt[OBS_MAX_MULTIPLIERS * D + e]) / (TIn)dt[(OBS_MAX_MULTIPLIERS + 1) * D + e];
}

// frame `s` (num_stack - 1: the current one) of element `e` on one lane after this launch, with the history brought up to date:
// a launch that shifts moves frame s + 1 into frame s, one that does not keeps the older frames; a lane of `reset_mask` restarts
// them from zero.  An element that is not stacked has no history.
template<class TIn, class TOut>
JM_DEV TIn observe_frame(const int32_t * __restrict__ it, const double * __restrict__ dt, const ObserveIO<TIn, TOut> & io, int D, int S,
                         int e, int s, bool shift, bool reset, long long B, long long lane)
{
    const bool stacked = it[OBS_IT_ELEM + OBS_ELEM_INTS * e + 2] != 0;
    TIn * h = io.hist + ((long long)s * D + e) * B + lane;
    if (s == S - 1)
    {
        const TIn x = observe_value<TIn, TOut>(it, dt, io, D, e, B, lane);
        if (stacked) *h = x;
        return x;
    }
    if (!stacked) return TIn(0);
    const TIn x = reset ? TIn(0) : (shift ? h[(long long)D * B] : *h);
    if (shift || reset) *h = x;
    return x;
}

#ifndef JM_HOST_EMU
// One block: 64 elements x 64 lanes, 4 waves.  Pass `s` of the stack: wave w computes the frame of the elements w, w + 4, ... for
// its 64 lanes (the element is uniform in the wave, so the plan is read through scalar loads and the sources and the history are
// read lane after lane) into `tile[element][lane]`; then thread t takes the element t % 64 and the lanes w, w + 4, ... out of
// the tile and writes `out[lane][position]`: consecutive threads, consecutive positions of a leaf.  The tile row is padded by
// one element: the transposed read of f32 then steps 65 dwords (bank (t + l) % 32, distinct in a half wave) and that of f64
// 130 dwords (bank (2 t + 2 l) % 64, distinct pairs in a half wave); the row writes are consecutive dwords.
template<class TIn, class TOut>
__global__ void __launch_bounds__(256) k_observe(const int32_t * __restrict__ it, const double * __restrict__ dt,
                                                  const ObserveIO<TIn, TOut> io, int shift, long long B)
{
    __shared__ TOut tile[OBS_TILE][OBS_TILE + 1];
    const int D = it[1], S = it[2], W = it[3];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), li = (int)(threadIdx.x & 63);
    const long long lane0 = (long long)blockIdx.x * OBS_TILE, lane = lane0 + li;
    const int e0 = (int)blockIdx.y * OBS_TILE;
    const bool live = lane < B;
    const bool reset = live && io.reset_mask && io.reset_mask[lane] != 0;
    const int32_t * pos = it + obs_it_pos(D);
    for (int s = 0; s < S; ++s)
    {
        for (int k = wave; k < OBS_TILE; k += 4)
        {
            const int e = e0 + k;
            if (e < D && live)
                tile[k][li] = (TOut)observe_frame<TIn, TOut>(it, dt, io, D, S, e, s, shift != 0, reset, B, lane);
        }
        __syncthreads();
        const int p = e0 + li < D ? pos[(long long)s * D + e0 + li] : -1;
        if (p >= 0)
            for (int l = wave; l < OBS_TILE; l += 4)
                if (lane0 + l < B) io.out[(lane0 + l) * W + p] = tile[li][l];
        __syncthreads();
    }
}
#endif
}  // namespace jm
