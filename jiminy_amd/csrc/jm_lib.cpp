// jm_lib.cpp -- C ABI (include/jiminy_hip.h) of the per-topology HIP library, compiled with
// `hipcc --offload-arch=gfx950 -x hip -DJM_TOPO_HEADER="topo_<hash>.h"` (jiminy_amd/codegen.py).
//
// The library owns only the model constants (host copy + one small device block per batch).
// All batch state is borrowed from the caller as raw device pointers; nothing is allocated
// inside start/step/dynamics (mirrors the reference's "no malloc during step" guarantee,
// core/unit/engine_sanity_check.cc:118-121).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#ifndef JM_TOPO_HEADER
#error "JM_TOPO_HEADER must name the generated topology header"
#endif
#include JM_TOPO_HEADER

#include "jm_kernels.h"
#include "jm_constraint.h"
#include "jm_qcon.h"
#include "jm_pack.h"
#include "jm_adaptive.h"
#include "jm_qdopri.h"
#include "jm_dispatch.h"
#include "jm_error.h"

#define JM_ABI_VERSION 11

#ifdef JM_SPLIT_CONSTRAINT
// the constraint-model kernel is instantiated by jm_lib_constraint.cpp (compiled in parallel)
namespace jm
{
extern template __global__ void k_constrained<double, Topo, false>(const BatchArgs<double>, const ConArgs<double>);
#if !JM_TOPO_QUAD
extern template __global__ void k_batch<double, Topo, true>(const BatchArgs<double>);
extern template __global__ void k_constrained<double, Topo, true>(const BatchArgs<double>, const ConArgs<double>);
#endif
#if JM_TOPO_QUAD
extern template __global__ void k_quad_con<double, Topo, 0>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_quad_con<double, Topo, 1>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_quad_gen<double, Topo>(const BatchArgs<double>);
extern template __global__ void k_quad_con_gen<double, Topo, 0>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_quad_con_gen<double, Topo, 1>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_quad_dopri<double, Topo>(const BatchArgs<double>, const AdaptiveArgs<double>, int);
extern template __global__ void k_quad_dopri_gen<double, Topo>(const BatchArgs<double>, const AdaptiveArgs<double>, int);
#endif
#if JM_TOPO_QCON_SPLIT
extern template __global__ void k_quad_con_split<double, Topo, 1, 0>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_quad_con_split<double, Topo, 2, 0>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_quad_con_split<double, Topo, 1, 1>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_quad_con_split<double, Topo, 2, 1>(const BatchArgs<double>, const QConArgs<double>);
extern template __global__ void k_qcon_pgs<double, Topo, 8, 0, JM_QCON_PGS_DEPTH>(const QConArgs<double>, const double *, unsigned);
extern template __global__ void k_qcon_pgs<double, Topo, 12, 64, JM_QCON_PGS_DEPTH - 1>(const QConArgs<double>, const double *, unsigned);
extern template __global__ void k_qtip_pgs<double, Topo>(const QConArgs<double>, const double *, unsigned);
extern template __global__ void k_qcon_pgs_lane<double, Topo>(const QConArgs<double>, const double *, int32_t *);
extern template __global__ void k_qcon_exact<double, Topo>(const QConArgs<double>);
extern template __global__ void k_qtip_exact<double, Topo>(const QConArgs<double>);
#endif
}
#endif

struct jm_model
{
    std::vector<double> params;  // Layout<Topo>, options tail = defaults
    bool root_at_origin = true;  // placement of joint 1 is the identity (limb-parallel kernel)
};

namespace jd = jm::dispatch;

struct jm_batch
{
    int variant = jd::FAMILY_LANE;
    const jm_model * model = nullptr;
    long long B = 0;
    int dtype = JM_F64;
    int device = 0;
    std::vector<double> params;
    void * d_params = nullptr;
    void * field[JM_F_COUNT] = {};
    bool started = false;
    bool qcon_split = true;   // constraint model, large solves: split step launches (JIMINY_AMD_QCON_SPLIT=0 at creation: single kernel)
    bool qcon_split_start = true;   // ... and split start / reset launches (JIMINY_AMD_QCON_SPLIT_START=0: single kernel)
    bool joint_locks = false; // the batch carries user-registered JointConstraints (jm_batch_set_joint_locks)
    // split stepping of robots whose solve runs one lane per robot (jm_qcon.h, qcon_pgs_lane): that kernel counts into one of four
    // slots, the history turns the counters of steps <= n - 2 into the form of step n (jm_dispatch.h); made by jm_batch_create
    jd::SplitHistory history;
    int32_t * lane_stat = nullptr;        // device, [SLOTS][4]
    int32_t * lane_stat_host = nullptr;   // pinned, [SLOTS][4]
    hipEvent_t lane_ev[jd::SplitHistory::SLOTS] = {};
    bool debug_split = false, split_capture = false;   // JM_DEBUG_SPLIT (print the counters as they are absorbed), JIMINY_AMD_QCON_SPLIT_CAPTURE (a captured step may take the split form) at creation
    // adaptive stepper: caller-owned workspace / per-lane state, library-owned active-lane counter
    void * ad_ws = nullptr;
    double * ad_fs = nullptr;
    int32_t * ad_is = nullptr;
    int32_t * ad_count = nullptr;       // device
    int32_t * ad_flags = nullptr;       // device, compact constraint flags [NF][B] (constraint model + adaptive)
    double * ad_stage_time = nullptr;   // device, [B]: time of the coming stage evaluation of every lane (process forces, per-stage form)
    // compact-batch overrides of the constraint state pointers (adaptive stepper), null = bound fields
    int32_t * ov_flags = nullptr; void * ov_data = nullptr; void * ov_ws = nullptr;
    int32_t * ad_count_host = nullptr;  // pinned host
    // constraint contact model (jm_constraint.h)
    jm_constraint_options copt = {JM_CONTACT_SPRING_DAMPER, 100, 0.0, 20.0, 1.0e-3, 1.0e-5, 1.0e-4, -1.0};
    // optional per-environment variation (GEN kernels): height map, frames of the applied wrenches
    const void * ground_h = nullptr;
    int ground_nx = 0, ground_ny = 0;
    double ground_x0 = 0, ground_y0 = 0, ground_dx = 1, ground_dy = 1;
    int applied_k = 0;
    double applied_p[12] = {0};
    int applied_joint[4] = {1, 1, 1, 1};
    // process forces (jm_batch_set_process_forces): spline components of the applied wrenches the kernels evaluate themselves
    int proc_k = 0;
    jm_process_force proc[4] = {};
    int proc_off = 0;   // where their block (jm::ProcBlock) sits in the parameter block
    int n_cus = 256;   // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    // per-launch timing with HIP events recorded on the launch stream (bench.py roofline leg)
    bool timing = false;
    std::vector<hipEvent_t> ev;  // pairs (begin, end), ring of JM_TIMING_RING launches
    size_t n_timed = 0;
};
#define JM_TIMING_RING 2048

namespace
{
int32_t upload_params(jm_batch * b);
// the description of the process forces the kernels read (jm::ProcBlock): the tail of the parameter block; pointers as bit patterns
int32_t write_process_block(jm_batch * b)
{
    auto bits = [](const void * p) { double x; static_assert(sizeof(x) == sizeof(p), "64-bit pointers"); std::memcpy(&x, &p, sizeof(x)); return x; };
    double * blk = b->params.data() + b->proc_off;
    for (int i = 0; i < jm::JM_PROC_BLOCK; ++i) blk[i] = 0.0;
    blk[0] = (double)b->proc_k;
    blk[1] = bits(b->field[JM_F_LANE_TIME]);
    blk[26] = bits(b->ad_stage_time);
    for (int i = 0; i < b->proc_k; ++i)
    {
        double * c = blk + 2 + 6 * i;
        c[0] = (double)b->proc[i].row; c[1] = (double)b->proc[i].n_knots; c[2] = b->proc[i].knot_spacing; c[3] = b->proc[i].scale;
        c[4] = bits(b->proc[i].values); c[5] = bits(b->proc[i].grads);
    }
    return upload_params(b);
}
int32_t upload_params(jm_batch * b)
{
    HIP_TRY(hipSetDevice(b->device));
    const size_t n = b->params.size();
    if (b->dtype == JM_F64)
    {
        HIP_TRY(hipMemcpy(b->d_params, b->params.data(), n * sizeof(double), hipMemcpyHostToDevice));
    }
    else
    {
        std::vector<float> pf(n);
        for (size_t i = 0; i < n; ++i) pf[i] = (float)b->params[i];
        HIP_TRY(hipMemcpy(b->d_params, pf.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
    return JM_OK;
}

// rows of the caller-owned constraint workspace: overflow of the per-robot solver region (branch-parallel
// kernel) or the dense per-lane delassus workspace (one-robot-per-lane kernel)
template<class Tp> int32_t constraint_ws_rows_of(const jm_batch * b)
{
    if constexpr (Tp::QUAD)
        if (b->variant == jd::FAMILY_QUAD)
        {
            int rows = jm::qcon_ws_rows<double, Tp>();
            if constexpr (jm::qcon_split<Tp>())
                if (jm::qcon_split_ws_rows<double, Tp>() > rows) rows = jm::qcon_split_ws_rows<double, Tp>();
            return rows > 0 ? rows : 1;
        }
    return jm::ConRows<Tp>::WTOTAL;
}
int32_t constraint_ws_rows(const jm_batch * b) { return constraint_ws_rows_of<Topo>(b); }

template<class T> jm::BatchArgs<T> make_args(const jm_batch * b)
{
    jm::BatchArgs<T> A;
    std::memset(&A, 0, sizeof(A));
    A.P = (const T *)b->d_params;
    A.q = (T *)b->field[JM_F_Q];
    A.v = (T *)b->field[JM_F_V];
    A.a = (T *)b->field[JM_F_A];
    A.command = (const T *)b->field[JM_F_COMMAND];
    A.u_motor = (T *)b->field[JM_F_U_MOTOR];
    A.u = (T *)b->field[JM_F_U];
    A.f_external = (T *)b->field[JM_F_F_EXTERNAL];
    A.contact_forces = (T *)b->field[JM_F_CONTACT_FORCES];
    A.imu = (T *)b->field[JM_F_IMU];
    A.force = (T *)b->field[JM_F_FORCE];
    A.contact = (T *)b->field[JM_F_CONTACT];
    A.encoder = (T *)b->field[JM_F_ENCODER];
    A.effort = (T *)b->field[JM_F_EFFORT];
    A.energy = (T *)b->field[JM_F_ENERGY];
    A.joint_forces = (T *)b->field[JM_F_JOINT_FORCES];
    A.centroidal = (T *)b->field[JM_F_CENTROIDAL];
    A.status = (int32_t *)b->field[JM_F_STATUS];
    A.ws = (T *)b->field[JM_F_WORKSPACE];
    A.B = b->B;
    A.model_lane = (const T *)b->field[JM_F_MODEL_LANE];
    A.ground_h = (const T *)b->ground_h;
    A.ground_nx = b->ground_nx; A.ground_ny = b->ground_ny;
    A.ground_x0 = (T)b->ground_x0; A.ground_y0 = (T)b->ground_y0; A.ground_dx = (T)b->ground_dx; A.ground_dy = (T)b->ground_dy;
    A.ground_off = b->ground_h ? (const T *)b->field[JM_F_GROUND_OFFSET] : nullptr;
    A.applied = b->applied_k > 0 ? (const T *)b->field[JM_F_APPLIED] : nullptr;
    // process forces: float64 tables (refused on a float32 batch by select_form), with or without held rows
    const bool proc = b->proc_k > 0 && b->applied_k > 0 && std::is_same<T, double>::value;
    A.applied_k = (A.applied || proc) ? b->applied_k : 0;
    A.proc_off = proc ? b->proc_off : 0;   // (their description: the tail of the parameter block, write_process_block)
    for (int i = 0; i < 12; ++i) A.applied_p[i] = (T)b->applied_p[i];
    for (int i = 0; i < 4; ++i) A.applied_joint[i] = b->applied_joint[i];
    // spring-damper model: the lane's own friction coefficient when the field is bound (variation kernels)
    A.friction = b->copt.contact_model == JM_CONTACT_CONSTRAINT ? nullptr : (const T *)b->field[JM_F_FRICTION];
    A.flex_lane = (const T *)b->field[JM_F_FLEXIBILITY];
    return A;
}

template<class T, class Tp> constexpr jd::Traits traits_of()
{
    if constexpr (Tp::QUAD) return {true, jm::qcon_split<Tp>(), jm::qcon_split_large<Tp>(), jm::quad_block_waves<T, Tp>(), jm::qcon_split_lane<Tp>()};
    else return {false, false, false, 1, false};
}

// run-time facts of a launch (jm_dispatch.h) but for the stream's capture state and the verdict of the history
template<class T> jd::Facts facts_of(const jm_batch * b, const jm::BatchArgs<T> & A)
{
    jd::Facts f = {};
    f.mode = A.mode; f.f64 = std::is_same<T, double>::value; f.family = b->variant;
    f.constraint = b->copt.contact_model == JM_CONTACT_CONSTRAINT; f.con_rows = jm::ConRows<Topo>::NR > 0;
    f.model_lane = A.model_lane; f.ground = A.ground_h; f.applied = A.applied; f.friction = A.friction;
    f.joint_locks = b->joint_locks; f.compact = b->ov_flags; f.B = A.B; f.n_cus = b->n_cus;
    f.torsion = b->copt.torsion >= 2.220446049250313e-16;   // (four-row contact blocks: never the fixed layout)
    f.process = b->proc_k > 0;
    f.split = b->qcon_split; f.split_start = b->qcon_split_start; f.split_capture = b->split_capture;
    return f;
}

// the history once it has taken in the counters of the steps <= n - 2 that are still out (long arrived: no stall)
const jd::SplitHistory & drained_history(jm_batch * b)
{
    for (int k = b->history.due(); k >= 0; k = b->history.due())
    {
        (void)hipEventSynchronize(b->lane_ev[k]);
        const int32_t * st = b->lane_stat_host + 4 * k;
        if (b->debug_split) std::fprintf(stderr, "[split] miss %d sweeps %d waves %d longest %d\n", st[0], st[1], st[2], st[3]);
        b->history.absorb(k, st);
    }
    return b->history;
}

// constraint contact model on the branch-parallel decomposition (jm_qcon.h): its arguments from those of the lane family
jm::QConArgs<double> qcon_args(const jm::BatchArgs<double> & A, const jm::ConArgs<double> & C0)
{
    jm::QConArgs<double> C;
    C.flags = C0.flags; C.data = C0.data; C.ws = C0.ws; C.friction = C0.friction;
    C.kp = C0.kp; C.kd = C0.kd; C.kp_lock = C0.kp_lock; C.kd_lock = C0.kd_lock; C.torsion = C0.torsion; C.reg = C0.reg; C.tol_abs = C0.tol_abs; C.tol_rel = C0.tol_rel;
    C.iter_max = C0.iter_max; C.ground_h = A.ground_h; C.ground_nx = A.ground_nx; C.ground_ny = A.ground_ny;
    C.ground_x0 = A.ground_x0; C.ground_y0 = A.ground_y0; C.ground_dx = A.ground_dx; C.ground_dy = A.ground_dy;
    C.stage = nullptr; C.split_e = 0; C.split_pass = 0; C.split_r0 = 0; C.split_r1 = (int)A.B;
    return C;
}

// streamed solve of the split forms: solves of up to 64 rows, then the waves that hold a larger one, then the waves whose
// robots all have few active joint rows (operational-space form, jm_qtip.h)
template<class Tp> void qcon_split_solve(const jm::BatchArgs<double> & A, const jm::QConArgs<double> & C, unsigned g64, hipStream_t s)
{
    hipLaunchKernelGGL((jm::k_qcon_pgs<double, Tp, 8, 0, JM_QCON_PGS_DEPTH>), dim3(g64), dim3(256), 0, s, C, A.P, (unsigned)A.B);
    if constexpr (jm::QConRows<Tp>::MAXM > 64)
        hipLaunchKernelGGL((jm::k_qcon_pgs<double, Tp, 12, 64, JM_QCON_PGS_DEPTH - 1>), dim3(g64), dim3(256), 0, s, C, A.P, (unsigned)A.B);
    if constexpr (jm::QTip<Tp>::ON)
        hipLaunchKernelGGL((jm::k_qtip_pgs<double, Tp>), dim3(g64), dim3(256), 0, s, C, A.P, (unsigned)A.B);
}

// Engine::start / reset as launches of the split kernels, the four passes of the initialisation (engine.cc:1399-1467): first
// pass (every constraint enabled, hysteresis, free acceleration with u = 0, matrix and right-hand side) | exact solve | three
// times (multipliers -> u, free acceleration, right-hand side | Gauss-Seidel) | closing evaluation with the outputs.  (The
// single kernel took 52-67 ms per launch at B = 32 768 whatever the number of lanes that restart: NOTES/LAB_NOTEBOOK.md.)
template<class Tp> void launch_split_start(const jm::BatchArgs<double> & A, jm::QConArgs<double> C, hipStream_t s)
{
    C.stage = C.ws + (size_t)jm::qcon_split_region_rows<double, Tp>() * (size_t)A.B;
    const unsigned g64 = (unsigned)((A.B + 63) / 64);
    hipLaunchKernelGGL((jm::k_quad_con_split<double, Tp, 1, 1>), dim3(g64), dim3(256), 0, s, A, C);
    hipLaunchKernelGGL((jm::k_qcon_exact<double, Tp>), dim3(g64), dim3(256), 0, s, C);
    if constexpr (jm::QTip<Tp>::ON)
        hipLaunchKernelGGL((jm::k_qtip_exact<double, Tp>), dim3((unsigned)((A.B + 255) / 256)), dim3(256), 0, s, C);
    for (int pass = 1; pass <= 3; ++pass)
    {
        C.split_pass = pass;
        hipLaunchKernelGGL((jm::k_quad_con_split<double, Tp, 1, 1>), dim3(g64), dim3(256), 0, s, A, C);
        qcon_split_solve<Tp>(A, C, g64, s);
    }
    C.split_pass = 4;
    hipLaunchKernelGGL((jm::k_quad_con_split<double, Tp, 2, 1>), dim3(g64), dim3(256), 0, s, A, C);
}

// step launches of the split form: pre | solve | post per evaluation (jm_qcon.h).  Robots whose system fits the fixed 16-row
// layout solve one lane per robot, out of registers (qcon_pgs_lane), and are marked done for the streamed form that follows;
// with `counters` that kernel counts into the history's slot of this step, read back behind the chain.
template<class Tp> void launch_split_step(jm_batch * b, const jm::BatchArgs<double> & A, jm::QConArgs<double> C, bool counters, hipStream_t s)
{
    const int slot = b->history.slot();
    int32_t * miss = counters ? b->lane_stat + 4 * slot : nullptr;
    if (miss) (void)hipMemsetAsync(miss, 0, 4 * sizeof(int32_t), s);
    C.stage = C.ws + (size_t)jm::qcon_split_region_rows<double, Tp>() * (size_t)A.B;
    const int n_evals = (A.command_changed ? 1 : 0) + A.n_sub * (A.solver == JM_SOLVER_RUNGE_KUTTA_4 ? 4 : 1);
    const unsigned g64 = (unsigned)((A.B + 63) / 64);
    for (int e = 0; e < n_evals; ++e)
    {
        C.split_e = e;
        hipLaunchKernelGGL((jm::k_quad_con_split<double, Tp, 1, 0>), dim3(g64), dim3(256), 0, s, A, C);
        if constexpr (jm::qcon_split_lane<Tp>())
            hipLaunchKernelGGL((jm::k_qcon_pgs_lane<double, Tp>), dim3(g64), dim3(64), 0, s, C, A.P, miss);
        qcon_split_solve<Tp>(A, C, g64, s);
        hipLaunchKernelGGL((jm::k_quad_con_split<double, Tp, 2, 0>), dim3(g64), dim3(256), 0, s, A, C);
    }
    if (miss)
    {
        (void)hipMemcpyAsync(b->lane_stat_host + 4 * slot, miss, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        (void)hipEventRecord(b->lane_ev[slot], s);
        b->history.recorded(slot);
    }
}

jm::ConArgs<double> con_args(const jm_batch * b)
{
    jm::ConArgs<double> C;
    C.flags = b->ov_flags ? b->ov_flags : (int32_t *)b->field[JM_F_CON_FLAGS];
    C.data = (double *)(b->ov_data ? b->ov_data : b->field[JM_F_CON_DATA]);
    C.ws = (double *)(b->ov_ws ? b->ov_ws : b->field[JM_F_WORKSPACE]);
    // per-lane friction: bound field (compact batches of the adaptive stepper read it through BatchArgs::lane_map)
    C.friction = (const double *)b->field[JM_F_FRICTION];
    const double omega = 2.0 * 3.14159265358979323846 * b->copt.stabilization_freq;  // abstract_constraint.cc:88-98
    C.kp = omega * omega; C.kd = 2.0 * omega;
    // user-registered constraints: gains of their own when the option says so (jm_constraint_options, ABI 6)
    const double omega_u = 2.0 * 3.14159265358979323846 * b->copt.user_stabilization_freq;
    C.kp_lock = b->copt.user_stabilization_freq < 0.0 ? C.kp : omega_u * omega_u;
    C.kd_lock = b->copt.user_stabilization_freq < 0.0 ? C.kd : 2.0 * omega_u;
    C.torsion = b->copt.torsion; C.reg = b->copt.regularization;
    C.tol_abs = b->copt.tol_abs; C.tol_rel = b->copt.tol_rel; C.iter_max = b->copt.pgs_iter_max;
    C.xl = nullptr; C.xstride = 0; C.yl = nullptr; C.ystride = 0; C.yrows = 0;  // set by the kernel (LDS)
    C.park = nullptr; C.park_rows = 0;
    return C;
}

// the kernels of a form; false when this topology has none (the `if constexpr` guards keep a topology from instantiating
// kernels it has no use for: a form whose guard is off is a defect of the selector, never a silent no-op).  The kernels are
// named in the order the compiler has always met them: the register allocation of some follows it
template<class T, class Tp> bool launch_form(jm_batch * b, const jm::BatchArgs<T> & A, const jd::Selection & sel, hipStream_t s)
{
    constexpr bool F64 = std::is_same<T, double>::value, SPLIT = traits_of<T, Tp>().qcon_split;
    constexpr int waves = traits_of<T, Tp>().block_waves;   // (the branch-parallel kernels: 4 lanes per robot)
    const dim3 grid((unsigned)((A.B + 63) / 64)), qgrid((unsigned)((A.B + 16 * waves - 1) / (16 * waves))), grid1((unsigned)((A.B + 15) / 16));
    // the constraint model.  Its single kernel on the branch-parallel decomposition: `start` / `reset` -- Engine::start's four
    // passes with the exact solve -- and the variation form (user JointConstraints too, unless the topology splits) are
    // instantiations of their own
    if constexpr (F64)
    {
        constexpr int cw = [] { if constexpr (Tp::QUAD) return jm::qcon_block_waves<double, Tp>(); else return 1; }();
        const dim3 cgrid((unsigned)((A.B + 16 * cw - 1) / (16 * cw)));
        const jm::ConArgs<double> C = con_args(b);
        const jm::QConArgs<double> Q = qcon_args(A, C);
        switch (sel.form)
        {
        case jd::SPLIT_START: if constexpr (SPLIT) launch_split_start<Tp>(A, Q, s); return SPLIT;
        case jd::SPLIT_STEP: case jd::SPLIT_STEP_LANE: if constexpr (SPLIT) launch_split_step<Tp>(b, A, Q, sel.counters, s); return SPLIT;
        case jd::QCON_GEN_INIT: if constexpr (Tp::QUAD) hipLaunchKernelGGL((jm::k_quad_con_gen<double, Tp, 1>), cgrid, dim3(64 * cw), 0, s, A, Q); return Tp::QUAD;
        case jd::QCON_GEN: if constexpr (Tp::QUAD) hipLaunchKernelGGL((jm::k_quad_con_gen<double, Tp, 0>), cgrid, dim3(64 * cw), 0, s, A, Q); return Tp::QUAD;
        case jd::QCON_INIT: if constexpr (Tp::QUAD) hipLaunchKernelGGL((jm::k_quad_con<double, Tp, 1>), cgrid, dim3(64 * cw), 0, s, A, Q); return Tp::QUAD;
        case jd::QCON: if constexpr (Tp::QUAD) hipLaunchKernelGGL((jm::k_quad_con<double, Tp, 0>), cgrid, dim3(64 * cw), 0, s, A, Q); return Tp::QUAD;
        case jd::LANE_CON_GEN: if constexpr (!Tp::QUAD) hipLaunchKernelGGL((jm::k_constrained<double, Tp, true>), grid, dim3(64), 0, s, A, C); return !Tp::QUAD;
        case jd::LANE_CON: hipLaunchKernelGGL((jm::k_constrained<double, Tp, false>), grid, dim3(64), 0, s, A, C); return true;
        default: break;
        }
    }
    switch (sel.form)
    {
    case jd::QUAD_GEN: if constexpr (Tp::QUAD && F64) hipLaunchKernelGGL((jm::k_quad_gen<T, Tp>), qgrid, dim3(64 * waves), 0, s, A); return Tp::QUAD && F64;
    case jd::QUAD_ONE_WAVE: if constexpr (Tp::QUAD && waves > 1) hipLaunchKernelGGL((jm::k_quad<T, Tp, 1>), grid1, dim3(64), 0, s, A); return Tp::QUAD && waves > 1;
    case jd::QUAD: if constexpr (Tp::QUAD) hipLaunchKernelGGL((jm::k_quad<T, Tp>), qgrid, dim3(64 * waves), 0, s, A); return Tp::QUAD;
    case jd::LANE_BATCH_GEN: if constexpr (F64 && !Tp::QUAD) hipLaunchKernelGGL((jm::k_batch<T, Tp, true>), grid, dim3(64), 0, s, A); return F64 && !Tp::QUAD;
    case jd::LANE_BATCH: hipLaunchKernelGGL((jm::k_batch<T, Tp, false>), grid, dim3(64), 0, s, A); return true;
    default: return false;
    }
}

// every launch of the model kernels: facts -> form (jm_dispatch.h) -> the kernels of that form
template<class T> int32_t launch(jm_batch * b, jm::BatchArgs<T> & A, void * stream)
{
    HIP_TRY(hipSetDevice(b->device));
    const hipStream_t s = (hipStream_t)stream;
    constexpr jd::Traits traits = traits_of<T, Topo>();
    jd::Facts f = facts_of<T>(b, A);
    // a simulation starts with a clean history: the forms of its steps depend on its data only
    if (A.mode == jm::MODE_START) b->history.reset();
    // a constraint step whose form the history chooses; a captured one neither reads nor advances it
    const bool lane_step = traits.lane_history() && f.f64 && f.constraint && f.con_rows && f.family == jd::FAMILY_QUAD && A.mode == jm::MODE_STEP;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    f.capturing = lane_step && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    const bool stepping = lane_step && !f.capturing;
    if (stepping) f.cooling = !drained_history(b).allowed();
    const jd::Selection sel = jd::select_form(traits, f);
    if (sel.form == jd::REFUSED) return fail(JM_ENOTIMPL, sel.refusal);
    if (f.constraint && f.con_rows && (!b->field[JM_F_CON_FLAGS] || !b->field[JM_F_CON_DATA] || !b->field[JM_F_WORKSPACE]))
        return fail(JM_ECONTROLFLOW, "contacts.model = 'constraint': the con_flags, con_data and workspace fields must be bound");
    if (stepping) (void)b->history.take_step();
    // only the step launches are timed: the roofline leg prices one pass of the hot path, not the
    // (cheaper, single-evaluation) start / reset / dynamics launches
    const bool timed = b->timing && A.mode == jm::MODE_STEP && b->n_timed < JM_TIMING_RING;
    if (timed) HIP_TRY(hipEventRecord(b->ev[2 * b->n_timed], s));
    if (!launch_form<T, Topo>(b, A, sel, s)) return fail(JM_ERUNTIME, "this library has no kernel for the selected form");
    HIP_TRY(hipGetLastError());
    if (timed)
    {
        HIP_TRY(hipEventRecord(b->ev[2 * b->n_timed + 1], s));
        ++b->n_timed;
    }
    return JM_OK;
}

// the float64 / float32 switch of the entry points: `f` gets a zero of the batch's scalar type ...
template<class F> int32_t with_dtype(const jm_batch * b, F && f) { return b->dtype == JM_F64 ? f(double()) : f(float()); }
// ... and the launches among them: the batch's arguments, `set` the mode and what goes with it, launch
template<class F> int32_t launch_as(jm_batch * b, void * stream, F && set)
{
    return with_dtype(b, [&](auto z) { auto A = make_args<decltype(z)>(b); set(A); return launch(b, A, stream); });
}

int32_t check_bound(const jm_batch * b, bool need_command)
{
    if (b->proc_k > 0)
    {
        if (!b->field[JM_F_LANE_TIME]) return fail(JM_ECONTROLFLOW, "process forces need the lane-time field (JM_F_LANE_TIME) bound");
        for (int i = 0; i < b->proc_k; ++i)
            if (b->proc[i].row >= 6 * b->applied_k)
                return fail(JM_ECONTROLFLOW, "a process force targets a frame that jm_batch_set_applied_frames did not register");
    }
    if (!b->field[JM_F_Q] || !b->field[JM_F_V] || !b->field[JM_F_A])
        return fail(JM_ECONTROLFLOW, "state fields q, v, a must be bound before this call");
    if (need_command && Topo::NM > 0 && !b->field[JM_F_COMMAND])
        return fail(JM_ECONTROLFLOW, "the command field must be bound before this call");
    return JM_OK;
}

template<class T> int32_t step_adaptive(jm_batch * b, double t_next, const jm_adaptive_options * o, int32_t new_step,
                                               int32_t command_changed, int32_t update_sensors, int32_t max_attempts,
                                               int32_t * attempts_out, void * stream)
{
    const hipStream_t s = (hipStream_t)stream;
    using R = jm::AdaptiveRows<Topo>;
    T * ws = (T *)b->ad_ws;
    const long long B = b->B;
    jm::AdaptiveArgs<T> D;
    D.P = (const T *)b->d_params;
    D.q = (T *)b->field[JM_F_Q]; D.v = (T *)b->field[JM_F_V]; D.a = (T *)b->field[JM_F_A];
    D.ws = ws; D.fs = b->ad_fs; D.is = b->ad_is; D.status = (int32_t *)b->field[JM_F_STATUS];
    D.n_active = b->ad_count; D.B = B;
    D.t_next = t_next; D.tol_rel = o->tol_rel; D.tol_abs = o->tol_abs; D.dt_max = o->dt_max;
    D.dt_restore_threshold_rel = o->dt_restore_threshold_rel; D.succ_failed_max = o->successive_iter_failed_max;
    D.new_step = new_step; D.stage = 0;
    // process forces: the per-stage kernels leave the time of every stage for the dynamics launch and advance the lanes' process time
    const bool proc = b->proc_k > 0 && b->applied_k > 0 && std::is_same<T, double>::value;
    D.lane_time = proc ? (T *)b->field[JM_F_LANE_TIME] : nullptr;
    D.stage_time = proc ? b->ad_stage_time : nullptr;
    if (D.status && new_step) HIP_TRY(hipMemsetAsync(D.status, 0, sizeof(int32_t) * B, s));
    // FSAL fix when the command changed at the breakpoint: a(t+) (engine.cc:2030-2042)
    if (command_changed)
    {
        auto A = make_args<T>(b);
        A.mode = jm::MODE_DYNAMICS; A.q_in = D.q; A.v_in = D.v; A.a_out = D.a;
        const int32_t rc = launch<T>(b, A, stream);
        if (rc != JM_OK) return rc;
    }
    D.command = (const T *)b->field[JM_F_COMMAND];
    D.n_act = B;  // upper bound of the active-list length: the list only shrinks within an interval
    const bool constrained = b->copt.contact_model == JM_CONTACT_CONSTRAINT && jm::ConRows<Topo>::NR > 0;
    D.con_flags = constrained ? (int32_t *)b->field[JM_F_CON_FLAGS] : nullptr;
    D.con_data = constrained ? (T *)b->field[JM_F_CON_DATA] : nullptr;
    D.con_flags_c = b->ad_flags;
    if (constrained && (!D.con_flags || !D.con_data || !b->ad_flags))
        return fail(JM_ECONTROLFLOW, "contacts.model = 'constraint': bind con_flags / con_data, then jm_batch_bind_adaptive");
    // the persistent form (jm_dispatch.h, select_adaptive_form): every quad runs its robot's whole adaptive loop on the chip; the
    // host only learns whether a robot ran into the attempt bound of a launch (then it launches again) and the largest attempt count
    auto A0 = make_args<T>(b);
    A0.mode = jm::MODE_DYNAMICS;
    jd::Facts facts = facts_of<T>(b, A0);
    facts.friction = b->field[JM_F_FRICTION];   // (alone it also needs the variation kernel: only its contact law reads the field)
    const jd::Form form = jd::select_adaptive_form(traits_of<T, Topo>(), facts, o->form == 1);
    if constexpr (Topo::QUAD && std::is_same<T, double>::value)
    {
        if (form != jd::DOPRI_STAGES)
        {
            constexpr int nth = 64 * jm::qdopri_block_waves<T, Topo>();
            const unsigned grid = (unsigned)((B + nth / 4 - 1) / (nth / 4));
            const int per_launch = 4096;
            int total = 0;
            for (;;)
            {
                HIP_TRY(hipMemsetAsync(b->ad_count, 0, 2 * sizeof(int32_t), s));
                if (form == jd::DOPRI_GEN) hipLaunchKernelGGL((jm::k_quad_dopri_gen<T, Topo>), dim3(grid), dim3(nth), 0, s, A0, D, per_launch);
                else hipLaunchKernelGGL((jm::k_quad_dopri<T, Topo>), dim3(grid), dim3(nth), 0, s, A0, D, per_launch);
                HIP_TRY(hipGetLastError());
                D.new_step = 0;
                HIP_TRY(hipMemcpyAsync(b->ad_count_host, b->ad_count, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                total += b->ad_count_host[1];
                if (b->ad_count_host[0] == 0) break;
                if (total >= max_attempts) return fail(JM_ERUNTIME, "adaptive stepper: too many attempts for one breakpoint interval");
            }
            if (attempts_out) *attempts_out = total;
            auto Ar = make_args<T>(b);
            Ar.mode = jm::MODE_REFRESH; Ar.update_sensors = update_sensors;
            return launch<T>(b, Ar, stream);
        }
    }
    const unsigned g256 = (unsigned)((B + 255) / 256);
    int attempts = 0;
    for (;;)
    {
        // all lanes: step-size selection + the list of the lanes that still have to move
        HIP_TRY(hipMemsetAsync(b->ad_count, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL((jm::k_dopri_prepare<T, Topo>), dim3(g256), dim3(256), 0, s, D);
        D.new_step = 0;
        HIP_TRY(hipMemcpyAsync(b->ad_count_host, b->ad_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const long long n = *b->ad_count_host;
        if (n == 0) break;
        if (attempts >= max_attempts) return fail(JM_ERUNTIME, "adaptive stepper: too many attempts for one breakpoint interval");
        // The n active lanes only: compact workspace rows [rows][n], dense batch of n robots for the dynamics
        // kernels.  Short lists are launch-bound: several attempts are then issued per synchronisation, the
        // grids and row strides stay sized for n while the kernels read the current length on the device.
        D.n_act = n;
        const int burst = n > 16384 ? 1 : (n > 2048 ? 3 : 8);
        const unsigned g128 = (unsigned)((n + 127) / 128);
        for (int k = 0; k < burst; ++k, ++attempts)
        {
            if (k > 0)
            {
                HIP_TRY(hipMemsetAsync(b->ad_count, 0, sizeof(int32_t), s));
                hipLaunchKernelGGL((jm::k_dopri_prepare<T, Topo>), dim3(g256), dim3(256), 0, s, D);
            }
            for (int i = 1; i <= 6; ++i)
            {
                D.stage = i;
                hipLaunchKernelGGL((jm::k_dopri_stage<T, Topo>), dim3(g128), dim3(128), 0, s, D);
                auto A = make_args<T>(b);
                A.mode = jm::MODE_DYNAMICS;
                A.B = n;
                A.command = ws + (long long)R::CMD * n;
                A.q_in = ws + (long long)R::QS * n;
                A.v_in = ws + (long long)(R::KV + (i - 1) * Topo::NV) * n;
                A.a_out = ws + (long long)(R::KA + (i - 1) * Topo::NV) * n;
                // (per-lane optional inputs -- body parameters, friction, applied wrenches, terrain patch -- stay in batch order)
                A.lane_map = b->ad_is + (long long)jm::AD_MAP * b->B;
                A.B_full = b->B;
                if (constrained)
                {
                    b->ov_flags = b->ad_flags;
                    b->ov_data = ws + (long long)R::CDATA * n;
                    b->ov_ws = ws + (long long)R::CWS * n;
                }
                const int32_t rc = launch<T>(b, A, stream);
                b->ov_flags = nullptr; b->ov_data = nullptr; b->ov_ws = nullptr;
                if (rc != JM_OK) return rc;
            }
            hipLaunchKernelGGL((jm::k_dopri_finish<T, Topo>), dim3(g128), dim3(128), 0, s, D);
            HIP_TRY(hipGetLastError());
        }
    }
    if (attempts_out) *attempts_out = attempts;
    // extra terms + sensors at the breakpoint (engine.cc:2148, 2386-2410)
    auto A = make_args<T>(b);
    A.mode = jm::MODE_REFRESH; A.update_sensors = update_sensors;
    return launch<T>(b, A, stream);
}
}  // namespace

extern "C"
{
const char * jm_topology_signature(void) { return Topo::signature; }
int32_t jm_abi_version(void) { return JM_ABI_VERSION; }

int32_t jm_model_create(const jm_model_desc * desc, jm_model ** out)
{
    if (!desc || !out) return fail(JM_EINVAL, "jm_model_create: null argument");
    std::string why;
    if (!jm::check_topology<Topo>(*desc, why)) return fail(JM_ETOPOLOGY, why);
    jm_model * m = new (std::nothrow) jm_model();
    if (!m) return fail(JM_ERUNTIME, "out of host memory");
    m->params = jm::pack_model<Topo>(*desc);
    jm::pack_options<Topo>(m->params, jm::default_options());
    jm::pack_quad<Topo>(m->params, *desc);
    if (desc->njoints > 1)
    {
        static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int k = 0; k < 9; ++k) m->root_at_origin &= (desc->placement_R[9 + k] == I9[k]);
        for (int k = 0; k < 3; ++k) m->root_at_origin &= (desc->placement_p[3 + k] == 0.0);
    }
    *out = m;
    return JM_OK;
}
int32_t jm_model_destroy(jm_model * model)
{
    delete model;
    return JM_OK;
}

int32_t jm_batch_create(const jm_model * model, int64_t batch_size, int32_t dtype, int32_t device, jm_batch ** out)
{
    if (!model || !out) return fail(JM_EINVAL, "jm_batch_create: null argument");
    if (batch_size <= 0) return fail(JM_EINVAL, "batch size must be positive");
    // kernels address every field with unsigned 32-bit element offsets (row * B + lane)
    {
        const long long max_rows = 6LL * (Topo::NJ > Topo::NC ? Topo::NJ : Topo::NC) + Topo::NQ + 16;
        if (batch_size * max_rows >= (1LL << 29))
            return fail(JM_EINVAL, "batch too large for one jm_batch (32-bit field offsets): shard it over several batches");
    }
    if (dtype != JM_F64 && dtype != JM_F32) return fail(JM_EINVAL, "dtype must be JM_F64 or JM_F32");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(JM_EINVAL, "invalid HIP device ordinal");
    jm_batch * b = new (std::nothrow) jm_batch();
    if (!b) return fail(JM_ERUNTIME, "out of host memory");
    b->model = model;
    b->B = batch_size;
    b->dtype = dtype;
    b->device = device;
    b->params = model->params;
    b->proc_off = (int)b->params.size();
    b->params.resize(b->params.size() + jm::JM_PROC_BLOCK, 0.0);
    // kernel variant: limb-parallel when the topology allows it; JM_KERNEL_VARIANT=lane forces the
    // generic one-robot-per-lane kernel (A/B measurements)
    b->variant = (Topo::QUAD && model->root_at_origin) ? jd::FAMILY_QUAD : jd::FAMILY_LANE;
    // (`start` / `reset` of robots with small solves: the single kernel -- its passes run on chip; jm_qcon.h, k_quad_con<1>)
    if constexpr (Topo::QUAD) b->qcon_split_start = jm::qcon_split_large<Topo>();
    if (const char * e = std::getenv("JIMINY_AMD_QCON_SPLIT")) b->qcon_split = e[0] != '0';
    if (const char * e = std::getenv("JIMINY_AMD_QCON_SPLIT_START")) b->qcon_split_start = e[0] != '0';
    b->debug_split = std::getenv("JM_DEBUG_SPLIT") != nullptr; b->split_capture = std::getenv("JIMINY_AMD_QCON_SPLIT_CAPTURE") != nullptr;
    if (const char * v = std::getenv("JM_KERNEL_VARIANT"))
        if (std::string(v) == "lane") b->variant = jd::FAMILY_LANE;
    hipError_t e = hipSetDevice(device);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) b->n_cus = cus;
    }
    if (e == hipSuccess) e = hipMalloc(&b->d_params, b->params.size() * sizeof(double));
    // counters of the one-lane-per-robot solve, their pinned mirror and events (a failure frees them with the batch)
    constexpr size_t stat_bytes = 4 * jd::SplitHistory::SLOTS * sizeof(int32_t);
    const bool counters = traits_of<double, Topo>().lane_history();
    if (e == hipSuccess && counters) e = hipMalloc((void **)&b->lane_stat, stat_bytes);
    if (e == hipSuccess && counters) e = hipHostMalloc((void **)&b->lane_stat_host, stat_bytes, hipHostMallocDefault);
    for (hipEvent_t & ev : b->lane_ev) if (e == hipSuccess && counters) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess && counters) std::memset(b->lane_stat_host, 0, stat_bytes);
    if (e != hipSuccess)
    {
        jm_batch_destroy(b);
        return fail(JM_ERUNTIME, std::string("jm_batch_create: ") + hipGetErrorString(e));
    }
    const int32_t rc = upload_params(b);
    if (rc != JM_OK)
    {
        jm_batch_destroy(b);
        return rc;
    }
    *out = b;
    return JM_OK;
}
int32_t jm_batch_destroy(jm_batch * b)
{
    if (!b) return JM_OK;
    (void)hipSetDevice(b->device);
    if (b->d_params) (void)hipFree(b->d_params);
    if (b->ad_count) (void)hipFree(b->ad_count);
    if (b->lane_stat) (void)hipFree(b->lane_stat);
    if (b->lane_stat_host) (void)hipHostFree(b->lane_stat_host);
    for (hipEvent_t e : b->lane_ev) if (e) (void)hipEventDestroy(e);
    if (b->ad_flags) (void)hipFree(b->ad_flags);
    if (b->ad_stage_time) (void)hipFree(b->ad_stage_time);
    if (b->ad_count_host) (void)hipHostFree(b->ad_count_host);
    for (hipEvent_t e : b->ev) (void)hipEventDestroy(e);
    delete b;
    return JM_OK;
}
int32_t jm_batch_set_joint_locks(jm_batch * b, int32_t on)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_set_joint_locks: null batch");
    // (both kernel families read bit 2 of the constraint flags; the branch-parallel one also selects its general sweep form by this switch)
    b->joint_locks = on != 0;
    return JM_OK;
}
int32_t jm_batch_set_options(jm_batch * b, const jm_options * o)
{
    if (!b || !o) return fail(JM_EINVAL, "jm_batch_set_options: null argument");
    if (b->started)
        return fail(JM_ECONTROLFLOW, "options cannot be changed while a simulation is running");  // engine.cc:2656-2662
    if (!(o->contact_stiffness >= 0.0) || !(o->contact_damping >= 0.0) || !(o->contact_friction >= 0.0))
        return fail(JM_EINVAL, "contact stiffness, damping and friction must be non-negative");
    if (!(o->contact_transition_velocity > 0.0)) return fail(JM_EINVAL, "contacts.transitionVelocity must be positive");
    if (o->contact_transition_eps < 0.0) return fail(JM_EINVAL, "contacts.transitionEps must be non-negative");  // engine.cc:2697-2702
    jm::pack_options<Topo>(b->params, *o);
    return upload_params(b);
}
int32_t jm_batch_workspace_rows(const jm_batch * b)
{
    return (b && b->copt.contact_model == JM_CONTACT_CONSTRAINT) ? constraint_ws_rows(b) : 0;
}
int32_t jm_batch_set_constraint_options(jm_batch * b, const jm_constraint_options * o)
{
    if (!b || !o) return fail(JM_EINVAL, "jm_batch_set_constraint_options: null argument");
    if (b->started)
        return fail(JM_ECONTROLFLOW, "options cannot be changed while a simulation is running");  // engine.cc:2656-2662
    if (o->contact_model != JM_CONTACT_SPRING_DAMPER && o->contact_model != JM_CONTACT_CONSTRAINT)
        return fail(JM_EINVAL, "The requested contact model is not available.");  // engine.cc:2741-2747
    if (!(o->regularization >= 0.0)) return fail(JM_EINVAL, "Constraint option 'regularization' must be positive.");
    if (!(o->stabilization_freq >= 0.0)) return fail(JM_EINVAL, "Contact option 'stabilizationFreq' must be positive.");
    if (!(o->torsion >= 0.0)) return fail(JM_EINVAL, "contacts.torsion must be non-negative");
    if (!(o->tol_abs > 0.0) || !(o->tol_rel > 0.0)) return fail(JM_EINVAL, "tolAbs and tolRel must be positive");
    if (o->pgs_iter_max <= 50) return fail(JM_EINVAL, "pgs_iter_max must exceed 50 (relaxation schedule of the PGS solver)");
    // one-robot-per-lane kernel with 64-bit row offsets into the workspace; the batch must still fit
    b->copt = *o;
    return JM_OK;
}
int32_t jm_batch_constraint_rows(const jm_batch * b, int32_t * n_flag_rows, int32_t * n_data_rows, int32_t * n_workspace_rows)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_constraint_rows: null batch");
    using R = jm::ConRows<Topo>;
    if (n_flag_rows) *n_flag_rows = R::NF;
    if (n_data_rows) *n_data_rows = R::ND;
    if (n_workspace_rows) *n_workspace_rows = constraint_ws_rows(b);
    return JM_OK;
}
int32_t jm_batch_set_ground(jm_batch * b, const void * heights, int32_t nx, int32_t ny, double x0, double y0, double dx, double dy)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_set_ground: null batch");
    if (heights && (nx < 2 || ny < 2 || !(dx > 0.0) || !(dy > 0.0)))
        return fail(JM_EINVAL, "jm_batch_set_ground: the height map needs at least 2 x 2 samples and positive spacings");
    b->ground_h = heights; b->ground_nx = nx; b->ground_ny = ny;
    b->ground_x0 = x0; b->ground_y0 = y0; b->ground_dx = dx; b->ground_dy = dy;
    return JM_OK;
}
int32_t jm_batch_set_applied_frames(jm_batch * b, int32_t k, const double * offsets, const int32_t * joints)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_set_applied_frames: null batch");
    if (k < 0 || k > 4 || (k > 0 && !offsets)) return fail(JM_EINVAL, "jm_batch_set_applied_frames: 0 <= K <= 4 frames with their offsets");
    for (int i = 0; i < k; ++i)
        if (joints && (joints[i] < 1 || joints[i] >= Topo::NJ)) return fail(JM_EINVAL, "jm_batch_set_applied_frames: parent joint out of range");
    b->applied_k = k;
    for (int i = 0; i < 3 * k; ++i) b->applied_p[i] = offsets[i];
    for (int i = 0; i < 4; ++i) b->applied_joint[i] = (joints && i < k) ? joints[i] : 1;
    return JM_OK;
}
int32_t jm_batch_set_process_forces(jm_batch * b, int32_t k, const jm_process_force * forces)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_set_process_forces: null batch");
    if (b->started)
        return fail(JM_ECONTROLFLOW, "A simulation is already running. Please stop it before changing the process forces.");
    if (k < 0 || k > 4 || (k > 0 && !forces)) return fail(JM_EINVAL, "jm_batch_set_process_forces: 0 <= K <= 4 process forces");
    for (int i = 0; i < k; ++i)
    {
        const jm_process_force & f = forces[i];
        if (f.row < 0 || f.row >= 24) return fail(JM_EINVAL, "jm_batch_set_process_forces: target row out of range (6 * frame + component, 4 frames)");
        if (f.n_knots < 1 || !(f.knot_spacing > 0.0)) return fail(JM_EINVAL, "jm_batch_set_process_forces: a process needs knots and a positive knot spacing");
        if (!f.values || !f.grads) return fail(JM_EINVAL, "jm_batch_set_process_forces: null table");
    }
    if (k > 0 && b->dtype != JM_F64) return fail(JM_ENOTIMPL, "process forces need a float64 batch");
    b->proc_k = k;
    for (int i = 0; i < 4; ++i) b->proc[i] = i < k ? forces[i] : jm_process_force{};
    return write_process_block(b);
}
int32_t jm_batch_bind(jm_batch * b, int32_t field, void * ptr)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_bind: null batch");
    if (field < 0 || field >= JM_F_COUNT) return fail(JM_ELOOKUP, "jm_batch_bind: unknown field id");
    b->field[field] = ptr;
    if (field == JM_F_LANE_TIME && b->proc_k > 0) return write_process_block(b);
    return JM_OK;
}

int32_t jm_batch_start(jm_batch * b, void * stream)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_start: null batch");
    int32_t rc = check_bound(b, true);
    if (rc != JM_OK) return rc;
    rc = launch_as(b, stream, [](auto & A) { A.mode = jm::MODE_START; });
    if (rc == JM_OK) b->started = true;
    return rc;
}

int32_t jm_batch_stop(jm_batch * b)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_stop: null batch");
    b->started = false;
    return JM_OK;
}

int32_t jm_batch_step(jm_batch * b, int32_t solver, double dt, int32_t n_substeps, int32_t command_changed,
                      int32_t update_sensors, void * stream)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_step: null batch");
    if (!b->started)
        return fail(JM_ECONTROLFLOW, "No simulation running. Please start one before using step method.");  // engine.cc:1727-1731
    if (solver != JM_SOLVER_EULER_EXPLICIT && solver != JM_SOLVER_RUNGE_KUTTA_4)
        return fail(JM_ENOTIMPL, "only 'euler_explicit' and 'runge_kutta_4' are available on the batched path");
    // (`dt` is the step of the integrator -- the inner loop of Engine::step, which goes down to STEPPER_MIN_TIMESTEP when what
    // is left of a breakpoint interval is that short, engine.cc:2047-2089 --, not the user-level step size, whose bound
    // SIMULATION_MIN_TIMESTEP <= step (engine.cc:1750-1753) is checked where the schedule is planned)
    if (!(dt >= 1e-10) || !(dt <= 0.02 + 1e-12))
        return fail(JM_EINVAL, "Step size out of bounds.");  // constants.h:18-20
    if (n_substeps < 1) return fail(JM_EINVAL, "n_substeps must be >= 1");
    int32_t rc = check_bound(b, true);
    if (rc != JM_OK) return rc;
    return launch_as(b, stream, [&](auto & A) {
        A.mode = jm::MODE_STEP; A.solver = solver; A.dt = (decltype(A.dt))dt; A.n_sub = n_substeps;
        A.command_changed = command_changed; A.update_sensors = update_sensors;
    });
}

// ---- adaptive Dormand-Prince stepping (jm_adaptive.h)
int32_t jm_batch_adaptive_workspace_rows(const jm_batch * b)
{
    return (b && b->copt.contact_model == JM_CONTACT_CONSTRAINT) ? jm::AdaptiveRows<Topo>::CWS + constraint_ws_rows(b)
                                                                 : jm::AdaptiveRows<Topo>::TOTAL;
}
int32_t jm_batch_bind_adaptive(jm_batch * b, void * workspace, double * state_f64, int32_t * state_i32)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_bind_adaptive: null batch");
    b->ad_ws = workspace; b->ad_fs = state_f64; b->ad_is = state_i32;
    if (!b->ad_count)
    {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipMalloc((void **)&b->ad_count, 2 * sizeof(int32_t)));
        if (jm::ConRows<Topo>::NF > 0)
            HIP_TRY(hipMalloc((void **)&b->ad_flags, sizeof(int32_t) * (size_t)jm::ConRows<Topo>::NF * (size_t)b->B));
        HIP_TRY(hipHostMalloc((void **)&b->ad_count_host, 2 * sizeof(int32_t), hipHostMallocDefault));
    }
    if (!b->ad_stage_time)
    {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipMalloc((void **)&b->ad_stage_time, sizeof(double) * (size_t)b->B));
        HIP_TRY(hipMemset(b->ad_stage_time, 0, sizeof(double) * (size_t)b->B));
        if (b->proc_k > 0) return write_process_block(b);
    }
    return JM_OK;
}
int32_t jm_batch_step_adaptive(jm_batch * b, double t_next, const jm_adaptive_options * options, int32_t new_step,
                               int32_t command_changed, int32_t update_sensors, int32_t max_attempts,
                               int32_t * attempts_out, void * stream)
{
    if (!b || !options) return fail(JM_EINVAL, "jm_batch_step_adaptive: null argument");
    if (!b->started)
        return fail(JM_ECONTROLFLOW, "No simulation running. Please start one before using step method.");
    if (!b->ad_ws || !b->ad_fs || !b->ad_is)
        return fail(JM_ECONTROLFLOW, "jm_batch_bind_adaptive must be called before the adaptive stepper is used");
    if (b->copt.contact_model == JM_CONTACT_CONSTRAINT && b->dtype != JM_F64)
        return fail(JM_ENOTIMPL, "contacts.model = 'constraint' needs a float64 batch");
    if (!(options->tol_rel > 0.0) || !(options->tol_abs > 0.0)) return fail(JM_EINVAL, "tolRel and tolAbs must be positive");
    if (!(options->dt_max >= 1e-6) || !(options->dt_max <= 0.02 + 1e-12)) return fail(JM_EINVAL, "'dtMax' option is out of range.");
    int32_t rc = check_bound(b, true);
    if (rc != JM_OK) return rc;
    HIP_TRY(hipSetDevice(b->device));
    return with_dtype(b, [&](auto z) {
        return step_adaptive<decltype(z)>(b, t_next, options, new_step, command_changed, update_sensors, max_attempts, attempts_out, stream);
    });
}

int32_t jm_batch_dynamics(jm_batch * b, const void * q_in, const void * v_in, void * a_out, void * stream)
{
    if (!b || !q_in || !v_in || !a_out) return fail(JM_EINVAL, "jm_batch_dynamics: null argument");
    if (!b->started)
        return fail(JM_ECONTROLFLOW, "No simulation running. Please start one before calling this method.");  // engine.cc:3594-3599
    if (Topo::NM > 0 && !b->field[JM_F_COMMAND]) return fail(JM_ECONTROLFLOW, "the command field must be bound");
    return launch_as(b, stream, [&](auto & A) {
        A.mode = jm::MODE_DYNAMICS; A.q_in = (decltype(A.q_in))q_in; A.v_in = (decltype(A.v_in))v_in; A.a_out = (decltype(A.a_out))a_out;
    });
}

int32_t jm_batch_reset_lanes(jm_batch * b, const uint8_t * lane_mask, const void * q_init, const void * v_init, void * stream)
{
    if (!b || !lane_mask || !q_init || !v_init) return fail(JM_EINVAL, "jm_batch_reset_lanes: null argument");
    if (!b->started) return fail(JM_ECONTROLFLOW, "No simulation running. Please start one before resetting lanes.");
    int32_t rc = check_bound(b, true);
    if (rc != JM_OK) return rc;
    return launch_as(b, stream, [&](auto & A) {
        A.mode = jm::MODE_RESET; A.mask = lane_mask; A.q_init = (decltype(A.q_init))q_init; A.v_init = (decltype(A.v_init))v_init;
    });
}

int32_t jm_batch_enable_timing(jm_batch * b, int32_t enable)
{
    if (!b) return fail(JM_EINVAL, "jm_batch_enable_timing: null batch");
    HIP_TRY(hipSetDevice(b->device));
    if (enable && b->ev.empty())
    {
        b->ev.resize(2 * JM_TIMING_RING, nullptr);
        for (hipEvent_t & e : b->ev) HIP_TRY(hipEventCreate(&e));
    }
    b->timing = enable != 0;
    b->n_timed = 0;
    return JM_OK;
}
int32_t jm_batch_timing_summary(jm_batch * b, int32_t * n_launches, double * total_ms)
{
    if (!b || !n_launches || !total_ms) return fail(JM_EINVAL, "jm_batch_timing_summary: null argument");
    double sum = 0.0;
    for (size_t i = 0; i < b->n_timed; ++i)
    {
        HIP_TRY(hipEventSynchronize(b->ev[2 * i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, b->ev[2 * i], b->ev[2 * i + 1]));
        sum += ms;
    }
    *n_launches = (int32_t)b->n_timed;
    *total_ms = sum;
    b->n_timed = 0;
    return JM_OK;
}

int32_t jm_last_error(char * buffer, size_t size)
{
    if (!buffer || size == 0) return JM_EINVAL;
    std::snprintf(buffer, size, "%s", g_last_error.c_str());
    return JM_OK;
}
}  // extern "C"
