// jm_centroidal.h -- the centroidal quantities of an arbitrary state `(q, v, a)` as one batched HIP kernel: the centre of mass,
// the centroidal momentum and its time derivative, in the row layout of the engine's `centroidal` field.  Every lane is one
// environment, arrays are `[rows][B]` like the physics state.  The physics kernels leave these rows behind for the engine's
// own state only; this kernel evaluates them for any other one -- the state of a reference trajectory.
//
// Reference: `pin.computeCentroidalMomentumTimeVariation` (python/jiminy_py/src/jiminy_py/dynamics.py:496-499, reached from
// `StateQuantity.refresh`, python/gym_jiminy/common/gym_jiminy/common/bases/quantities.py:1494-1518), whose results the
// engine's own `computeExtraTerms` (core/src/engine/engine.cc:800-905) states as `dh`, `fBody` shifted to the centre of mass:
// `dhg` is `I a + v x* I v` summed over the bodies, without gravity and without external forces.
//
// A body is a walk from the universe to its joint frame, in the segment tables of jm_frames.h and through its per-segment
// walker, with the accelerations carried along: the lane's state is one rotation, one position, two velocity and two
// acceleration vectors in registers, and no per-joint array.  Every body is walked on its own (a shared prefix such as the
// base is recomputed).  Per body, in world axes about the world origin, the kernel sums `m c`, `m vc`, `I_w w + c x m vc` and
// the time derivatives of the last two; at the end the momenta are shifted to the centre of mass.  All lanes interpret the
// same tables: their reads are indexed by loop counters only and become scalar loads.
#pragma once
#include "jm_frames.h"

namespace jm
{
// ---- the packed plan: `it` is that of `walks_pack` with one walk per body; `dt` holds the segments' doubles, then
// n_bodies x (mass, centre of mass 3, inertia about it xx xy xz yy yz zz) in the body's joint frame, then the total mass.
constexpr int CT_BODY_DOUBLES = 10;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool centroidal_pack(const jm_centroidal_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const char * caller = "jm_centroidal_plan_create";
    const std::string who = std::string(caller) + ": ";
    if (!d) { why = who + "null description"; return false; }
    if (!d->body_seg_start || !d->seg_kind || !d->seg_joint || !d->seg_q_index || !d->seg_v_index || !d->seg_rot ||
        !d->seg_trans || !d->seg_axis || !d->body_mass || !d->body_com || !d->body_inertia)
    { why = who + "null array in the description"; return false; }
    if (d->n_bodies <= 0) { why = who + "bad sizes"; return false; }
    const std::vector<int32_t> mode((size_t)d->n_bodies, FR_LOCAL);
    const jm_frames_desc walks = {d->n_bodies, d->nq, d->nv, d->njoints, d->body_seg_start, mode.data(), d->n_seg, d->seg_kind,
                                  d->seg_joint, d->seg_q_index, d->seg_v_index, d->seg_rot, d->seg_trans, d->seg_axis};
    if (!walks_pack(&walks, it, dt, why, caller, "body")) return false;
    double total = 0.0;
    for (int b = 0; b < d->n_bodies; ++b)
    {
        const std::string body = "body " + std::to_string(b);
        bool finite = std::isfinite(d->body_mass[b]);
        for (int k = 0; k < 3; ++k) finite &= std::isfinite(d->body_com[3 * b + k]);
        for (int k = 0; k < 6; ++k) finite &= std::isfinite(d->body_inertia[6 * b + k]);
        if (!finite) { why = who + body + " has a constant that is not finite"; return false; }
        if (d->body_mass[b] < 0.0) { why = who + body + " has a negative mass"; return false; }
        total += d->body_mass[b];
        dt.push_back(d->body_mass[b]);
        dt.insert(dt.end(), d->body_com + 3 * b, d->body_com + 3 * b + 3);
        dt.insert(dt.end(), d->body_inertia + 6 * b, d->body_inertia + 6 * b + 6);
    }
    if (!(total > 0.0)) { why = who + "the bodies have no mass"; return false; }
    dt.push_back(total);
    return true;
}

// The centroidal rows of one lane.  q `[nq][B]`; v, a `[nv][B]` in pinocchio's convention (spatial, in the joint's local
// frame), a or null; out `[15][B]`: com (3), hg (linear 3, angular 3: about the centre of mass, world axes), dhg (6), the
// last six zero without `a`.
template<class T>
JM_DEV void centroidal_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, const T * __restrict__ q,
                            const T * __restrict__ v, const T * __restrict__ a, T * __restrict__ out, long long B, long long lane)
{
    const int K = it[0], si = it[1];
    const int n_seg = it[2 + 3 * (K - 1)] + it[3 + 3 * (K - 1)];
    const double * bodies = dt + (long long)n_seg * FR_SEG_DOUBLES;
    V3<T> mc = zero3<T>(), P = zero3<T>(), L = zero3<T>(), dP = zero3<T>(), dL = zero3<T>();
    for (int b = 0; b < K; ++b)
    {
        const int s0 = it[2 + 3 * b], s1 = s0 + it[3 + 3 * b];
        FrameWalk<T> k = frame_walk_start<T>();
        for (int s = s0; s < s1; ++s)
            frame_walk_segment<T, true>(k, s == s0, dt + (long long)s * FR_SEG_DOUBLES, it + si + FR_SEG_INTS * s, q, v, a, nullptr,
                                        true, B, lane);
        const double * d = bodies + (long long)b * CT_BODY_DOUBLES;
        const T m = (T)d[0];
        const S3<T> I = {(T)d[4], (T)d[5], (T)d[6], (T)d[7], (T)d[8], (T)d[9]};
        // the body's centre of mass: position, velocity and acceleration in the world frame
        const V3<T> rc = k.R * v3((T)d[1], (T)d[2], (T)d[3]);
        const V3<T> c = k.p + rc, wr = cross(k.w, rc);
        const V3<T> mv = m * (k.pd + wr), ma = m * (k.pdd + cross(k.wd, rc) + cross(k.w, wr));
        const V3<T> Iw = k.R * (I * tmul(k.R, k.w));
        mc = mc + m * c;
        P = P + mv;
        L = L + Iw + cross(c, mv);
        dP = dP + ma;
        // (d/dt of c x m vc: vc x m vc vanishes)
        dL = dL + k.R * (I * tmul(k.R, k.wd)) + cross(k.w, Iw) + cross(c, ma);
    }
    const T inv_mass = T(1) / (T)bodies[(long long)K * CT_BODY_DOUBLES];
    const V3<T> com = inv_mass * mc;
    const V3<T> Lg = L - cross(com, P), dLg = dL - cross(com, dP);
    T * o = out + lane;
    o[0] = com.x; o[B] = com.y; o[2 * B] = com.z;
    o[3 * B] = P.x; o[4 * B] = P.y; o[5 * B] = P.z;
    o[6 * B] = Lg.x; o[7 * B] = Lg.y; o[8 * B] = Lg.z;
    const bool has = a != nullptr;
    o[9 * B] = has ? dP.x : T(0); o[10 * B] = has ? dP.y : T(0); o[11 * B] = has ? dP.z : T(0);
    o[12 * B] = has ? dLg.x : T(0); o[13 * B] = has ? dLg.y : T(0); o[14 * B] = has ? dLg.z : T(0);
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_centroidal_state(const FramesArgs p, const T * __restrict__ q, const T * __restrict__ v,
                                                           const T * __restrict__ a, const uint8_t * __restrict__ lane_mask,
                                                           T * __restrict__ centroidal, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (lane_mask && !lane_mask[lane]) return;
    centroidal_lane<T>(p.it, p.dt, q, v, a, centroidal, B, lane);
}
#endif
}  // namespace jm
