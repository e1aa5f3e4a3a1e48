// jm_dispatch.h -- which kernel, or chain of kernels, runs a call of the C ABI library: the policy of jm_lib.cpp and nothing
// that launches.  Plain C++17 without a HIP include: jm_lib.cpp launches what `select_form` says, and the CPU suite compiles
// this header on its own (tests/hostemu/dispatch.cpp, tests/test_dispatch_policy.py).
#pragma once

#include <cstdint>

namespace jm::dispatch
{
enum { FAMILY_LANE = 0, FAMILY_QUAD = 1 };                              // (jm_batch::variant)
enum { STEP = 0, START = 1, DYNAMICS = 2, RESET = 3, REFRESH = 4 };     // (= jm::MODE_*, jm_kernels.h)

enum Form   // every form a call can take
{
    REFUSED = 0,                                 // JM_ENOTIMPL, Selection::refusal says why
    LANE_BATCH, LANE_BATCH_GEN,                  // k_batch<T, Topo, false>, k_batch<double, Topo, true>
    LANE_CON, LANE_CON_GEN,                      // k_constrained<double, Topo, false / true>
    QUAD, QUAD_ONE_WAVE, QUAD_GEN,               // k_quad<T, Topo> (the topology's block waves), k_quad<T, Topo, 1>, k_quad_gen
    QCON, QCON_INIT, QCON_GEN, QCON_GEN_INIT,    // k_quad_con<., INIT = 0 / 1>, k_quad_con_gen<., 0 / 1>
    SPLIT_START,                                 // first pass | exact solve | 3 x (pass | Gauss-Seidel) | closing evaluation
    SPLIT_STEP, SPLIT_STEP_LANE,                 // per evaluation pre | solve | post; ... the one-lane-per-robot solve ahead of the streamed one
    DOPRI, DOPRI_GEN, DOPRI_STAGES               // persistent k_quad_dopri / k_quad_dopri_gen; per-stage launches (DYNAMICS calls of their own)
};

// compile-time facts of a topology (and of the scalar type, for the block waves)
struct Traits
{
    bool quad;               // Topo::QUAD: the branch-parallel kernels exist
    bool qcon_split;         // jm::qcon_split<Topo>(): constraint steps may run as pre | solve | post
    bool qcon_split_large;   // jm::qcon_split_large<Topo>(): solves that live in the workspace (Atlas)
    int block_waves;         // jm::quad_block_waves<T, Topo>()
    bool lane_pgs;           // jm::QLanePgs<Topo>::FITS: the split step opens its solve with k_qcon_pgs_lane
    // small solves: the form of a constraint step follows the history of that kernel's counters (SplitHistory)
    constexpr bool lane_history() const { return qcon_split && !qcon_split_large; }
};

// run-time facts of one launch
struct Facts
{
    int mode, family, n_cus;
    long long B;                        // robots of the launch (a compact batch: the active ones)
    bool f64, constraint, con_rows;     // float64 batch; contacts.model = 'constraint'; the topology has constraint rows (ConRows::NR > 0)
    bool model_lane, ground, applied;   // optional inputs bound: per-lane body parameters, height map, applied wrenches
    bool friction;                      // per-lane friction the contact law of the launch reads (null under the constraint model)
    bool joint_locks, compact;          // user-registered JointConstraints; compact-batch overrides in use (adaptive per-stage launches)
    bool capturing, torsion;            // the stream is being captured into a graph; contacts.torsion >= eps (four-row contact blocks)
    bool split, split_start, split_capture;   // JIMINY_AMD_QCON_SPLIT, _SPLIT_START, _SPLIT_CAPTURE as read at creation
    bool cooling;                       // verdict of the history: this step stays with the single kernel (!SplitHistory::allowed())
    bool process = false;               // process forces registered (jm_batch_set_process_forces): spline wrench components the kernels evaluate
};

// `counters`, SPLIT_STEP*: the solve counts into a slot of the history
struct Selection { Form form; bool counters; const char * refusal; };

// THE predicate "this launch needs the variation (`_gen`) kernels".  Optional inputs: every family.  Per-lane friction: the
// branch-parallel spring-damper law only (the one-robot-per-lane kernels read it as it is, the constraint solvers as well).  Joint
// locks: the branch-parallel constraint kernels of topologies that never step in the split form (jm::qcon_locks).
constexpr bool needs_variation(const Traits & t, const Facts & f)
{
    if (f.model_lane || f.ground || f.applied || f.process) return true;
    if (f.family != FAMILY_QUAD) return false;
    return (f.constraint && f.con_rows) ? (f.joint_locks && !t.qcon_split) : f.friction;
}

constexpr Selection select_form(const Traits & t, const Facts & f)
{
    const bool quad = t.quad && f.family == FAMILY_QUAD;
    // body parameters per lane, height maps, applied wrenches: float64 instantiations of their own in either family (the
    // one-robot-per-lane ones exist for the topologies that have no branch-parallel kernels)
    const bool own = f.f64 && (quad || !t.quad);
    if (f.ground && !own) return {REFUSED, false, "a height-map ground needs a float64 batch (and, on a branch-parallel topology, its own kernels)"};
    if (f.model_lane && !own) return {REFUSED, false, "per-lane body parameters need a float64 batch (and, on a branch-parallel topology, its own kernels)"};
    if (f.friction && quad && !f.f64) return {REFUSED, false, "per-lane friction on a branch-parallel topology needs a float64 batch"};
    if (f.applied && !own) return {REFUSED, false, "applied wrenches need a float64 batch (and, on a branch-parallel topology, its own kernels)"};
    if (f.process && !own) return {REFUSED, false, "process forces need a float64 batch (and, on a branch-parallel topology, its own kernels)"};
    // constraint model, float64 only: the reference's precision; its PGS tolerances are below float32 round-off
    if (f.constraint && !f.f64) return {REFUSED, false, "contacts.model = 'constraint' needs a float64 batch"};
    const bool gen = needs_variation(t, f);
    const bool init = f.mode == START || f.mode == RESET;
    if (f.constraint && quad && f.con_rows)
    {
        // split forms: plain inputs, whole waves of 16 robots, never a compact batch
        const bool fits = t.qcon_split && f.split && !(f.model_lane || f.applied || f.process || f.ground) && (f.B & 15) == 0 && !f.compact;
        if (fits && init && f.split_start) return {SPLIT_START, false, nullptr};
        // small solves (one lane per robot): only while every solve of the batch fits that form and the solves are long (the
        // history decides); a captured step keeps one form for all its replays, the single kernel; torsion rows never fit
        const bool lane_ok = !t.lane_history() || !(f.cooling || (f.capturing && !f.split_capture) || f.torsion);
        if (fits && f.mode == STEP && lane_ok)
            return {t.lane_pgs ? SPLIT_STEP_LANE : SPLIT_STEP, t.lane_history() && !f.capturing, nullptr};
        return {gen ? (init ? QCON_GEN_INIT : QCON_GEN) : (init ? QCON_INIT : QCON), false, nullptr};
    }
    if (f.constraint) return {!t.quad && gen ? LANE_CON_GEN : LANE_CON, false, nullptr};
    if (!quad) return {!t.quad && f.f64 && gen ? LANE_BATCH_GEN : LANE_BATCH, false, nullptr};
    if (gen) return {QUAD_GEN, false, nullptr};
    // small batch: one wave per block so that the waves spread over all the CUs (the per-block limb table is a few kB, staging
    // it four times as often is noise next to idle CUs)
    const long long grid = (f.B + 16 * t.block_waves - 1) / (16 * t.block_waves);
    return {t.block_waves > 1 && grid < 2LL * f.n_cus ? QUAD_ONE_WAVE : QUAD, false, nullptr};
}

// adaptive stepper: branch-parallel topologies, spring-damper contacts, float64 run ONE persistent launch per interval
// (jm_qdopri.h) unless the caller asks for the per-stage launches.  `f.friction`: the field is bound.
constexpr Form select_adaptive_form(const Traits & t, const Facts & f, bool per_stage)
{
    if (!(t.quad && f.family == FAMILY_QUAD && f.f64) || (f.constraint && f.con_rows) || per_stage) return DOPRI_STAGES;
    return needs_variation(t, f) ? DOPRI_GEN : DOPRI;
}

// History of the one-lane-per-robot solve.  The solve kernel counts, per split step, [0] the robots it cannot take, [1] its
// sweeps, [2] its waves, [3] its longest solve.  A batch with misfits, or whose solves are short (robots standing under
// control), steps with the single kernel for a while, then steps in the split form probe again.  The decision for step n only
// reads the counters of steps <= n - 2 (long arrived: the wait does not stall), and `start` resets the state: the sequence of
// forms is a function of the simulated data, not of host timing -- two runs from the same state are bit-identical.
struct SplitHistory
{
    static constexpr int SLOTS = 4;
    long long step = 0;                            // split-capable step launches since `start`
    int cooldown = 0;                              // single-kernel steps still to run
    long long step_of[SLOTS] = {-1, -1, -1, -1};   // step whose counters the slot is waiting for (-1: free)
    void reset() { *this = SplitHistory(); }
    // oldest outstanding slot of a step <= n - 2, -1 when none is due
    int due() const
    {
        int k = -1;
        for (int i = 0; i < SLOTS; ++i)
            if (step_of[i] >= 0 && step_of[i] <= step - 2 && (k < 0 || step_of[i] < step_of[k])) k = i;
        return k;
    }
    void absorb(int slot, const int32_t * st)
    {
        step_of[slot] = -1;
        int cool = 0;
        if (st[0] > 0) cool = 64;
        // measured on ANYmal, 65 536 robots, per evaluation: single kernel ~147 us + 5.3 us per average sweep (its waves queue
        // four deep on a SIMD); split form ~247 us + 1.55 us per sweep of the LONGEST solve of the launch (every wave of the
        // solve kernel is resident at once)
        else if (st[2] > 0 && 5.3 * (double)st[1] / (double)st[2] - 1.55 * (double)st[3] < 100.0) cool = 256;
        if (cool > cooldown) cooldown = cool;
    }
    // the step about to be launched: may it take the split form?  `take_step` answers the same and moves on to the next step
    bool allowed() const { return cooldown == 0; }
    bool take_step()
    {
        const bool ok = allowed();
        if (!ok) --cooldown;
        ++step;
        return ok;
    }
    // slot a split step (the one `take_step` just allowed) counts into (drained before: its last step is <= n - 4)
    int slot() const { return (int)((step - 1) % SLOTS); }
    void recorded(int slot) { step_of[slot] = step - 1; }
};
}  // namespace jm::dispatch
