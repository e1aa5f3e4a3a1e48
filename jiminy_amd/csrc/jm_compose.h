// jm_compose.h -- the composition layer of the reference's gym environments as one batched HIP kernel: the termination
// conditions of `ComposedJiminyEnv(terminations=[...])` in their short-circuit order and the reward tree of
// `ComposedJiminyEnv(reward=...)` (additive L^p / L^inf mixtures, geometric means, `SurviveReward`, leaves), evaluated on the
// rows other blocks left on the device.  Every lane is one environment, arrays are `[rows][B]` like the physics state.  The
// kernel depends on no topology: what it reads is a table of base pointers handed over at launch and a packed plan.
//
// Reference (python/gym_jiminy/common/gym_jiminy/common):
//   AbstractReward.__call__, QuantityReward.compute, MixtureReward.compute      bases/compositions.py:177-228, :309-335, :412-438
//   AbstractTerminationCondition.__call__, QuantityTermination.compute          bases/compositions.py:540-574, :647-663
//   _array_contains                                                             utils/spaces.py:81-104
//   weighted_norm, geometric_mean                                               compositions/mixin.py:70-105, :203-222
//   SurviveReward.compute                                                       compositions/generic.py:55-61
//   ComposedJiminyEnv.has_terminated                                            bases/pipeline.py:751-797
//
// Three behaviours of the reference that the kernel reproduces:
//   1. a node is evaluated when `bool(is_terminal) == terminated`: an indefinite node (`is_terminal` None, which a mixture of
//      terminal and non-terminal components is) counts as non-terminal, and is skipped as a whole on a terminated lane;
//   2. an array-valued quantity fires on a NaN element (`not (low <= value).all()`), a 0-d quantity does not (`low > value`);
//   3. the max of the L^inf norm is Python's: `max(total, x)` is `x > total ? x : total`, which keeps `total` where `x` is NaN.
#pragma once
#include "jm_locomotion.h"

namespace jm
{
constexpr int CMP_MAX_SOURCES = 16, CMP_MAX_NODES = 32, CMP_MAX_DEPTH = 4, CMP_MAX_CONDITIONS = 16, CMP_MAX_ELEMENTS = 64;
// element kinds of a source
constexpr int CMP_SRC_DTYPE = 0, CMP_SRC_INT32 = 1, CMP_SRC_UINT8 = 2;
// node kinds
constexpr int CMP_LEAF = 0, CMP_SURVIVE = 1, CMP_ADDITIVE = 2, CMP_MULTIPLICATIVE = 3;
// flags of a condition, of an element
constexpr int CMP_COND_ARRAY = 1, CMP_COND_TRUNCATION = 2, CMP_COND_TRAINING_ONLY = 4;
constexpr int CMP_HAS_LOW = 1, CMP_HAS_HIGH = 2;
// ---- the packed plan, every table at a fixed offset.  `it`: [n_sources, n_nodes, n_conditions, n_elements, n_children, 0, 0,
// 0 | kind, rows of the 16 sources | 8 ints of each of the 32 nodes: kind, is_terminal (1 / 0 / -1 indefinite), is_normalized,
// slot, row, first child entry, number of children, order is infinite | 32 child entries (node indices) | 3 ints of each of the
// 16 conditions: first element, number of elements, flags | 3 ints of each of the 64 elements: slot, row, bound flags].
// `dt`: [order, 1 / order of the 32 nodes | weight of the 32 child entries | grace period of the 16 conditions | low, high of
// the 64 elements].  The root of the reward tree is node 0 and a child has a larger index than its parent.
constexpr int CMP_IT_SRC_KIND = 8, CMP_IT_SRC_ROWS = CMP_IT_SRC_KIND + CMP_MAX_SOURCES, CMP_IT_NODE = CMP_IT_SRC_ROWS + CMP_MAX_SOURCES,
              CMP_NODE_INTS = 8, CMP_IT_CHILD = CMP_IT_NODE + CMP_NODE_INTS * CMP_MAX_NODES, CMP_IT_COND = CMP_IT_CHILD + CMP_MAX_NODES,
              CMP_COND_INTS = 3, CMP_IT_ELEM = CMP_IT_COND + CMP_COND_INTS * CMP_MAX_CONDITIONS, CMP_ELEM_INTS = 3,
              CMP_IT_SIZE = CMP_IT_ELEM + CMP_ELEM_INTS * CMP_MAX_ELEMENTS;
constexpr int CMP_DT_ORDER = 0, CMP_DT_INV_ORDER = CMP_MAX_NODES, CMP_DT_WEIGHT = 2 * CMP_MAX_NODES, CMP_DT_GRACE = 3 * CMP_MAX_NODES,
              CMP_DT_LOW = CMP_DT_GRACE + CMP_MAX_CONDITIONS, CMP_DT_HIGH = CMP_DT_LOW + CMP_MAX_ELEMENTS,
              CMP_DT_SIZE = CMP_DT_HIGH + CMP_MAX_ELEMENTS;

inline bool compose_pack(const jm_compose_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_compose_plan_create: ";
    const auto no = [&](const std::string & what) { why = who + what; return false; };
    const auto at = [](const char * what, int i) { return std::string(what) + " " + std::to_string(i); };
    if (!d) return no("null description");
    if (d->n_sources < 0 || d->n_sources > CMP_MAX_SOURCES) return no("at most 16 sources are supported, got " + std::to_string(d->n_sources));
    if (d->n_nodes < 0 || d->n_nodes > CMP_MAX_NODES) return no("at most 32 reward nodes are supported, got " + std::to_string(d->n_nodes));
    if (d->n_conditions < 0 || d->n_conditions > CMP_MAX_CONDITIONS)
        return no("at most 16 termination conditions are supported, got " + std::to_string(d->n_conditions));
    if (d->n_elements < 0 || d->n_elements > CMP_MAX_ELEMENTS)
        return no("at most 64 termination elements are supported, got " + std::to_string(d->n_elements));
    if (d->n_children < 0 || d->n_children > CMP_MAX_NODES) return no("bad sizes: the number of child entries");
    if ((d->n_sources > 0 && (!d->source_kind || !d->source_rows)) ||
        (d->n_nodes > 0 && (!d->node_kind || !d->node_terminal || !d->node_normalized || !d->node_slot || !d->node_row ||
                            !d->node_child_start || !d->node_child_count || !d->node_order)) ||
        (d->n_children > 0 && (!d->child || !d->child_weight)) ||
        (d->n_conditions > 0 && (!d->cond_elem_start || !d->cond_elem_count || !d->cond_flags || !d->cond_grace)) ||
        (d->n_elements > 0 && (!d->elem_slot || !d->elem_row || !d->elem_bounds || !d->elem_low || !d->elem_high)))
        return no("null array in the description");
    it.assign(CMP_IT_SIZE, 0);
    dt.assign(CMP_DT_SIZE, 0.0);
    it[0] = d->n_sources; it[1] = d->n_nodes; it[2] = d->n_conditions; it[3] = d->n_elements; it[4] = d->n_children;
    for (int s = 0; s < d->n_sources; ++s)
    {
        if (d->source_kind[s] < CMP_SRC_DTYPE || d->source_kind[s] > CMP_SRC_UINT8)
            return no(at("source", s) + " has an element kind other than 0 (engine dtype), 1 (int32), 2 (uint8)");
        if (d->source_rows[s] < 1) return no(at("source", s) + " has no rows");
        it[CMP_IT_SRC_KIND + s] = d->source_kind[s];
        it[CMP_IT_SRC_ROWS + s] = d->source_rows[s];
    }
    const auto cell = [&](const std::string & who_, int slot, int row, std::string & msg) {
        if (slot < 0 || slot >= d->n_sources)
        { msg = who_ + " reads slot " + std::to_string(slot) + ", out of range [0, " + std::to_string(d->n_sources) + ")"; return false; }
        if (row < 0 || row >= d->source_rows[slot])
        { msg = who_ + " reads row " + std::to_string(row) + ", out of range [0, " + std::to_string(d->source_rows[slot]) + ") of its slot";
          return false; }
        return true;
    };
    std::string msg;
    // the reward tree: node 0 is the root, every other node is the child of exactly one node of a smaller index
    int depth[CMP_MAX_NODES] = {1}, parents[CMP_MAX_NODES] = {0};
    for (int n = 0; n < d->n_nodes; ++n)
    {
        int32_t * node = &it[CMP_IT_NODE + CMP_NODE_INTS * n];
        const int kind = d->node_kind[n];
        if (kind < CMP_LEAF || kind > CMP_MULTIPLICATIVE) return no(at("node", n) + " has an unknown kind");
        if (n > 0 && parents[n] != 1) return no(at("node", n) + " is not the child of exactly one node: the nodes do not form a tree");
        if (d->node_terminal[n] < -1 || d->node_terminal[n] > 1) return no(at("node", n) + ": is_terminal must be 1, 0 or -1 (indefinite)");
        node[0] = kind; node[1] = d->node_terminal[n]; node[2] = d->node_normalized[n] != 0;
        if (kind == CMP_LEAF)
        {
            if (!cell(at("node", n), d->node_slot[n], d->node_row[n], msg)) return no(msg);
            node[3] = d->node_slot[n]; node[4] = d->node_row[n];
        }
        if (kind != CMP_ADDITIVE && kind != CMP_MULTIPLICATIVE) continue;
        const int start = d->node_child_start[n], count = d->node_child_count[n];
        if (count < 1) return no("At least one reward component must be specified.");      // (bases/compositions.py:374-376)
        if (start < 0 || start > d->n_children - count) return no(at("node", n) + " has child entries out of range");
        if (depth[n] >= CMP_MAX_DEPTH) return no(at("node", n) + " has children below the depth of 4 levels that the kernel evaluates");
        node[5] = start; node[6] = count;
        if (kind == CMP_ADDITIVE)
        {
            const double p = d->node_order[n];
            if (!(p > 0.0)) return no("'order' must be strictly positive or 'inf'.");       // (compositions/mixin.py:149-150)
            node[7] = p > 1.7e308;
            dt[CMP_DT_ORDER + n] = node[7] ? 1.0 : p;
            dt[CMP_DT_INV_ORDER + n] = node[7] ? 1.0 : 1.0 / p;
        }
        for (int k = start; k < start + count; ++k)
        {
            const int c = d->child[k];
            if (c < 0 || c >= d->n_nodes) return no(at("node", n) + " has child " + std::to_string(c) + ", out of range [0, " +
                                                    std::to_string(d->n_nodes) + ")");
            if (c <= n) return no(at("node", n) + " has child " + std::to_string(c) + ": a cycle (a child has a larger index than its parent)");
            if (kind == CMP_ADDITIVE && !(d->child_weight[k] > 0.0)) return no(at("node", n) + " has a weight that is not positive");
            ++parents[c];
            depth[c] = depth[n] + 1;
            it[CMP_IT_CHILD + k] = c;
            dt[CMP_DT_WEIGHT + k] = d->child_weight[k];
        }
    }
    for (int c = 0; c < d->n_conditions; ++c)
    {
        const int start = d->cond_elem_start[c], count = d->cond_elem_count[c];
        if (count < 1 || start < 0 || start > d->n_elements - count) return no(at("condition", c) + " has elements out of range");
        if (d->cond_flags[c] & ~(CMP_COND_ARRAY | CMP_COND_TRUNCATION | CMP_COND_TRAINING_ONLY)) return no(at("condition", c) + " has unknown flags");
        if (!(d->cond_flags[c] & CMP_COND_ARRAY) && count != 1) return no(at("condition", c) + " is of the scalar form and has more than one element");
        if (d->cond_grace[c] != d->cond_grace[c]) return no(at("condition", c) + " has a grace period that is not a number");
        int32_t * cond = &it[CMP_IT_COND + CMP_COND_INTS * c];
        cond[0] = start; cond[1] = count; cond[2] = d->cond_flags[c];
        dt[CMP_DT_GRACE + c] = d->cond_grace[c];
    }
    for (int e = 0; e < d->n_elements; ++e)
    {
        if (!cell(at("element", e), d->elem_slot[e], d->elem_row[e], msg)) return no(msg);
        const int flags = d->elem_bounds[e];
        if (flags & ~(CMP_HAS_LOW | CMP_HAS_HIGH)) return no(at("element", e) + " has unknown bound flags");
        if (flags == (CMP_HAS_LOW | CMP_HAS_HIGH) && d->elem_low[e] > d->elem_high[e]) return no(at("element", e) + " has a low bound above its high bound");
        int32_t * elem = &it[CMP_IT_ELEM + CMP_ELEM_INTS * e];
        elem[0] = d->elem_slot[e]; elem[1] = d->elem_row[e]; elem[2] = flags;
        dt[CMP_DT_LOW + e] = (flags & CMP_HAS_LOW) ? d->elem_low[e] : 0.0;
        dt[CMP_DT_HIGH + e] = (flags & CMP_HAS_HIGH) ? d->elem_high[e] : 0.0;
    }
    return true;
}

template<class T> struct ComposeIO
{
    const void * source[CMP_MAX_SOURCES];   // base pointer of every slot, `[rows][B]` of the slot's element kind
    const T * time;                         // [B] the episode time of the lane (NULL: 0)
    const uint8_t * base_terminated;        // [B] (NULL: 0)
    const uint8_t * base_truncated;         // [B] (NULL: 0)
    const uint8_t * lane_mask;              // [B]
    T * reward;                             // [B]
    T * node_value;                         // [n_nodes][B], NaN where the node was not evaluated
    uint8_t * terminated;                   // [B]
    uint8_t * truncated;                    // [B]
    int32_t * trigger;                      // [B] the condition that fired; -1: none, or a base flag
    int32_t * violations;                   // [B] the bit of the first node advertised as normalised that left [0, 1]
};

// one element of a source as T; the slot is the same for every lane, so the pointer is picked by scalar selects and no table
// indexed at run time exists
template<class T>
JM_DEV T compose_load(const int32_t * __restrict__ it, const ComposeIO<T> & io, int slot, int row, long long B, long long lane)
{
    const void * base = io.source[0];
#pragma unroll
    for (int k = 1; k < CMP_MAX_SOURCES; ++k) base = slot == k ? io.source[k] : base;
    const long long o = (long long)row * B + lane;
    const int kind = it[CMP_IT_SRC_KIND + slot];
    if (kind == CMP_SRC_INT32) return (T)((const int32_t *)base)[o];
    if (kind == CMP_SRC_UINT8) return (T)((const uint8_t *)base)[o];
    return ((const T *)base)[o];
}

// ≙ `AbstractReward.__call__` of node `n`, whose subtree is at most D levels deep: its value where it was evaluated (`ok`),
// with the normalisation check and the `info` entry.  The accumulators of every level are locals of their own instantiation.
template<int D, class T>
JM_DEV T compose_node(const int32_t * __restrict__ it, const double * __restrict__ dt, const ComposeIO<T> & io, int n, bool terminated,
                      long long B, long long lane, bool & ok, uint32_t & violations)
{
    const int32_t * node = it + CMP_IT_NODE + CMP_NODE_INTS * n;
    const int kind = node[0];
    ok = false;
    T value = T(0);
    // (`bool(self.is_terminal) ^ terminated`: indefinite counts as non-terminal)
    if ((node[1] == 1) != terminated) return value;
    if (kind == CMP_LEAF)
    {
        value = compose_load<T>(it, io, node[3], node[4], B, lane);
        ok = true;
    }
    else if (kind == CMP_SURVIVE)
    {
        value = T(1);
        ok = true;
    }
    else
    {
        if constexpr (D > 1)
        {
            const int start = node[5], count = node[6];
            const bool additive = kind == CMP_ADDITIVE, is_max = node[7] != 0;
            const T order = (T)dt[CMP_DT_ORDER + n];
            T total = additive ? T(0) : T(1);
            int n_values = 0;
            for (int k = start; k < start + count; ++k)
            {
                bool child_ok;
                const T v = compose_node<D - 1, T>(it, dt, io, it[CMP_IT_CHILD + k], terminated, B, lane, child_ok, violations);
                if (!child_ok) continue;
                if (additive)
                {
                    const T w = (T)dt[CMP_DT_WEIGHT + k];
                    if (is_max)
                    {
                        const T x = w * v;
                        total = (n_values == 0 || x > total) ? x : total;      // (Python's `max(total, x)`)
                    }
                    else total += w * loco_pow(v, order);
                }
                else total *= v;
                ++n_values;
            }
            if (n_values > 0)
            {
                ok = true;
                if (additive) value = is_max ? total : loco_pow(total, (T)dt[CMP_DT_INV_ORDER + n]);
                else value = loco_pow(total, (T)(1.0 / (double)n_values));
            }
        }
    }
    if (!ok) return T(0);
    // (bases/compositions.py:216-218 raises; a lane records the first such node and goes on)
    if (node[2] && (value < T(0) || value > T(1)) && violations == 0u) violations = 1u << n;
    if (io.node_value) io.node_value[(long long)n * B + lane] = value;
    return value;
}

// ≙ `_array_contains` negated, for one element: the array form fires on NaN, the scalar form does not
template<class T> JM_DEV bool compose_out_of_bounds(T v, int flags, T low, T high, bool array_form)
{
    if (array_form) return ((flags & CMP_HAS_LOW) && !(low <= v)) || ((flags & CMP_HAS_HIGH) && !(v <= high));
    return ((flags & CMP_HAS_LOW) && low > v) || ((flags & CMP_HAS_HIGH) && v > high);
}

// Terminations, reward and normalisation check of one lane.  Every output may be null.
template<class T>
JM_DEV void compose_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, const ComposeIO<T> & io, bool training, long long B,
                         long long lane)
{
    const int n_nodes = it[1], n_conditions = it[2];
    bool terminated = io.base_terminated && io.base_terminated[lane] != 0, truncated = io.base_truncated && io.base_truncated[lane] != 0;
    int trigger = -1;
    if (!terminated && !truncated && n_conditions > 0)
    {
        const T t = io.time ? io.time[lane] : T(0);
        for (int c = 0; c < n_conditions; ++c)
        {
            const int32_t * cond = it + CMP_IT_COND + CMP_COND_INTS * c;
            const int flags = cond[2];
            if (((flags & CMP_COND_TRAINING_ONLY) && !training) || t < (T)dt[CMP_DT_GRACE + c]) continue;
            bool fired = false;
            for (int e = cond[0]; e < cond[0] + cond[1]; ++e)
            {
                const int32_t * elem = it + CMP_IT_ELEM + CMP_ELEM_INTS * e;
                const T v = compose_load<T>(it, io, elem[0], elem[1], B, lane);
                fired = fired || compose_out_of_bounds(v, elem[2], (T)dt[CMP_DT_LOW + e], (T)dt[CMP_DT_HIGH + e], (flags & CMP_COND_ARRAY) != 0);
            }
            if (fired)
            {
                terminated = !(flags & CMP_COND_TRUNCATION);
                truncated = !terminated;
                trigger = c;
                break;
            }
        }
    }
    if (io.terminated) io.terminated[lane] = terminated;
    if (io.truncated) io.truncated[lane] = truncated;
    if (io.trigger) io.trigger[lane] = trigger;
    uint32_t violations = 0u;
    T reward = T(0);
    if (n_nodes > 0)
    {
        if (io.node_value)
            for (int n = 0; n < n_nodes; ++n) io.node_value[(long long)n * B + lane] = T(__builtin_nan(""));
        bool ok;
        reward = compose_node<CMP_MAX_DEPTH, T>(it, dt, io, 0, terminated, B, lane, ok, violations);
    }
    if (io.reward) io.reward[lane] = reward;
    if (io.violations) io.violations[lane] = (int32_t)violations;
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_compose(const int32_t * __restrict__ it, const double * __restrict__ dt, const ComposeIO<T> io,
                                                  int training, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    compose_lane<T>(it, dt, io, training != 0, B, lane);
}
#endif
}  // namespace jm
