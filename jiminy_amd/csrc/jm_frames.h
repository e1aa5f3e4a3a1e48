// jm_frames.h -- frame kinematics as batched HIP kernels: the pose (position, quaternion, Euler angles) and the velocity of
// named frames from the lane's `q`, `v` -- what the reference reads from `pinocchio_data.oMf` and `getFrameVelocity` -- and
// the SE3 step average its quantity layer builds on them.  Every lane is one environment, arrays are `[rows][B]` like the
// physics state; the quaternion functions are those of jm_rotation.h.
//
// Reference (numpy code of python/gym_jiminy/common/gym_jiminy/common restated per lane):
//   xyzquat_difference                 utils/math.py:1009-1042
//   log6 / log3                        utils/math.py:842-894 / 725-774
//   exp6 / exp3                        utils/math.py:908-954 / 791-825
//   quat_multiply / quat_apply         utils/math.py:570-626 / 645-709
//   remove_yaw_from_quat               utils/math.py:1148-1198
//   AverageFrameXYZQuat.refresh        quantities/generic.py:1357-1360
//   FrameSpatialAverageVelocity.refresh    quantities/generic.py:1522-1534
//   BaseSpatialAverageVelocity.refresh     quantities/locomotion.py:281-288
// The reference differences and integrates poses with `pin.liegroups.SE3()`; utils/math.py documents `xyzquat_difference` as
// the same operation, and `integrate(p, w)` is `p` composed with `exp6(w)`.
//
// A frame is a walk from the universe to the frame, like `attitude_frame_rot` of jm_attitude.h with the translation and the
// velocity added: a list of segments, each a constant placement (rotation, translation) followed by the motion of one joint
// read from `q` and `v`.  Every frame is walked on its own (a shared prefix such as the base is recomputed): the per-lane
// state is one rotation, one position and two velocity vectors in registers.  All lanes interpret the same tables: their
// reads are indexed by loop counters only and become scalar loads.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "jm_rotation.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_frames, offset of the segment ints, n_frames x (first segment, segment count,
// mode), n_seg x (kind, joint, first q row, first v row)]; `dt` (float64) = n_seg x (9 rotation entries row-major,
// 3 translation entries, 3 axis entries).
constexpr int FR_SEG_DOUBLES = 15;
constexpr int FR_SEG_INTS = 4;
constexpr int FR_MAX_SEGS_PER_FRAME = 256;
// joint kinds of a segment (0 .. 6 as in jm_rotation.h, but 6 is the spherical joint alone)
constexpr int FR_FREEFLYER = 7, FR_PX = 8, FR_PAXIS = 11;
constexpr int FR_LOCAL = 0, FR_LOCAL_WORLD_ALIGNED = 1, FR_ODOMETRY = 2;
constexpr int MODEL_LANE_ROWS = 13, MODEL_LANE_PLACEMENT = 10;  // (JM_F_MODEL_LANE: translation of the placement of joint j)

// rows of `q` / `v` a joint kind reads
inline int frames_nq_of(int kind) { return kind == SEG_NONE ? 0 : kind == SEG_UNBOUNDED ? 2 : kind == SEG_QUAT ? 4 : kind == FR_FREEFLYER ? 7 : 1; }
inline int frames_nv_of(int kind) { return kind == SEG_NONE ? 0 : kind == SEG_QUAT ? 3 : kind == FR_FREEFLYER ? 6 : 1; }

// Validate a description of walks and pack it.  Returns false and a message on a malformed description.  `caller`, `noun`:
// the entry point and the name of a walk in the messages (jm_centroidal.h packs its bodies through here).
inline bool walks_pack(const jm_frames_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why,
                       const char * caller, const char * noun)
{
    const std::string who = std::string(caller) + ": ", frame = std::string(noun) + " ";
    if (!d) { why = who + "null description"; return false; }
    if (!d->frame_seg_start || !d->frame_mode || !d->seg_kind || !d->seg_joint || !d->seg_q_index || !d->seg_v_index ||
        !d->seg_rot || !d->seg_trans || !d->seg_axis)
    { why = who + "null array in the description"; return false; }
    if (d->n_frames <= 0 || d->n_seg <= 0 || d->nq < 0 || d->nv < 0 || d->njoints <= 0) { why = who + "bad sizes"; return false; }
    if (d->frame_seg_start[0] != 0 || d->frame_seg_start[d->n_frames] != d->n_seg)
    { why = who + noun + "_seg_start must run from 0 to n_seg"; return false; }
    for (int f = 0; f < d->n_frames; ++f)
    {
        const int n = d->frame_seg_start[f + 1] - d->frame_seg_start[f];
        if (n <= 0 || n > FR_MAX_SEGS_PER_FRAME)
        { why = who + frame + std::to_string(f) + " has a bad segment count (1 .. " + std::to_string(FR_MAX_SEGS_PER_FRAME) + ")"; return false; }
        if (d->frame_mode[f] < FR_LOCAL || d->frame_mode[f] > FR_ODOMETRY)
        { why = who + frame + std::to_string(f) + " has an unknown reference frame mode"; return false; }
    }
    for (int s = 0; s < d->n_seg; ++s)
    {
        const int kind = d->seg_kind[s], qi = d->seg_q_index[s], vi = d->seg_v_index[s], joint = d->seg_joint[s];
        const std::string seg = "segment " + std::to_string(s);
        if (kind < 0 || kind > FR_PAXIS) { why = who + seg + " has an unknown joint kind"; return false; }
        const int nq = frames_nq_of(kind), nv = frames_nv_of(kind);
        if (nq && (qi < 0 || qi + nq > d->nq))
        { why = who + seg + " reads q rows [" + std::to_string(qi) + ", " + std::to_string(qi + nq) + ") out of range [0, " +
                std::to_string(d->nq) + ")"; return false; }
        if (nv && (vi < 0 || vi + nv > d->nv))
        { why = who + seg + " reads v rows [" + std::to_string(vi) + ", " + std::to_string(vi + nv) + ") out of range [0, " +
                std::to_string(d->nv) + ")"; return false; }
        if (kind != SEG_NONE && (joint < 0 || joint >= d->njoints))
        { why = who + seg + " has joint index " + std::to_string(joint) + " out of range [0, " + std::to_string(d->njoints) + ")"; return false; }
        bool finite = true;
        for (int k = 0; k < 9; ++k) finite &= std::isfinite(d->seg_rot[9 * s + k]);
        for (int k = 0; k < 3; ++k) finite &= std::isfinite(d->seg_trans[3 * s + k]) && std::isfinite(d->seg_axis[3 * s + k]);
        if (!finite) { why = who + seg + " has a constant that is not finite"; return false; }
    }
    it.clear();
    it.push_back(d->n_frames);
    it.push_back(2 + 3 * d->n_frames);
    for (int f = 0; f < d->n_frames; ++f)
    {
        it.push_back(d->frame_seg_start[f]);
        it.push_back(d->frame_seg_start[f + 1] - d->frame_seg_start[f]);
        it.push_back(d->frame_mode[f]);
    }
    dt.clear();
    for (int s = 0; s < d->n_seg; ++s)
    {
        const bool none = d->seg_kind[s] == SEG_NONE;
        it.push_back(d->seg_kind[s]);
        it.push_back(none ? 0 : d->seg_joint[s]);
        it.push_back(none ? 0 : d->seg_q_index[s]);
        it.push_back(none ? 0 : d->seg_v_index[s]);
        dt.insert(dt.end(), d->seg_rot + 9 * s, d->seg_rot + 9 * s + 9);
        dt.insert(dt.end(), d->seg_trans + 3 * s, d->seg_trans + 3 * s + 3);
        dt.insert(dt.end(), d->seg_axis + 3 * s, d->seg_axis + 3 * s + 3);
    }
    return true;
}

// Validate the description of the frame kinematics and pack it.
inline bool frames_pack(const jm_frames_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    return walks_pack(d, it, dt, why, "jm_frames_plan_create", "frame");
}

// The state of a walk: world rotation and position, angular velocity and velocity of the origin in the world frame, and --
// for the walks that carry accelerations (jm_centroidal.h) -- the time derivatives of the two velocities.
template<class T> struct FrameWalk
{
    M3<T> R;
    V3<T> p, w, pd, wd, pdd;
};
template<class T> JM_DEV FrameWalk<T> frame_walk_start()
{
    return {ident3<T>(), zero3<T>(), zero3<T>(), zero3<T>(), zero3<T>(), zero3<T>()};
}

// One segment of a walk: the constant placement `d` (FR_SEG_DOUBLES), then the motion of the joint `is` (FR_SEG_INTS) names.
// `first`: the first segment of the walk (its rotation is the placement's).  `moving`: `w`, `pd` follow from `v`.  ACC (with
// `moving`): `wd`, `pdd` follow as well; `acc` `[nv][B]` holds the joint accelerations in pinocchio's convention (the time
// derivative of the rows of `v`), null: zeros, which leaves the velocity-product terms.
template<class T, bool ACC>
JM_DEV void frame_walk_segment(FrameWalk<T> & k, bool first, const double * __restrict__ d, const int * __restrict__ is,
                               const T * __restrict__ q, const T * __restrict__ v, const T * __restrict__ acc,
                               const T * __restrict__ model_lane, bool moving, long long B, long long lane)
{
    const int kind = is[0];
    V3<T> t = v3((T)d[9], (T)d[10], (T)d[11]);
    if (model_lane && kind != SEG_NONE)
    {
        const T * ml = model_lane + ((long long)is[1] * MODEL_LANE_ROWS + MODEL_LANE_PLACEMENT) * B + lane;
        t = v3(ml[0], ml[B], ml[2 * B]);
    }
    const V3<T> off = k.R * t;
    k.p = k.p + off;
    if (moving)
    {
        const V3<T> wo = cross(k.w, off);
        if (ACC) k.pdd = k.pdd + cross(k.wd, off) + cross(k.w, wo);
        k.pd = k.pd + wo;
    }
    const M3<T> Cm = {(T)d[0], (T)d[1], (T)d[2], (T)d[3], (T)d[4], (T)d[5], (T)d[6], (T)d[7], (T)d[8]};
    k.R = first ? Cm : k.R * Cm;
    if (kind == SEG_NONE) return;
    const T * qr = q + (long long)is[2] * B + lane;
    const T * vr = moving ? v + (long long)is[3] * B + lane : nullptr;
    const T * ar = ACC && moving && acc ? acc + (long long)is[3] * B + lane : nullptr;
    if (kind == SEG_QUAT || kind == FR_FREEFLYER)
    {
        // the velocity rows of both are expressed in the frame behind the joint (free-flyer: linear, then angular)
        if (kind == FR_FREEFLYER)
        {
            const V3<T> o2 = k.R * v3(qr[0], qr[B], qr[2 * B]);
            k.p = k.p + o2;
            if (moving)
            {
                const V3<T> wo = cross(k.w, o2);
                if (ACC) k.pdd = k.pdd + cross(k.wd, o2) + cross(k.w, wo);
                k.pd = k.pd + wo;
            }
            qr += 3 * B;
        }
        k.R = k.R * quat_to_matrix<T>(qr[0], qr[B], qr[2 * B], qr[3 * B]);
        if (moving)
        {
            V3<T> vl = zero3<T>();
            if (kind == FR_FREEFLYER)
            {
                vl = k.R * v3(vr[0], vr[B], vr[2 * B]);
                k.pd = k.pd + vl;
                vr += 3 * B;
            }
            const V3<T> wj = k.R * v3(vr[0], vr[B], vr[2 * B]);
            if (ACC)
            {
                // (the offset of a free-flyer turns with the frame in front of it, its velocity rows with the one behind)
                if (kind == FR_FREEFLYER)
                {
                    k.pdd = k.pdd + cross(k.w, vl) + cross(k.w + wj, vl);
                    if (ar) { k.pdd = k.pdd + k.R * v3(ar[0], ar[B], ar[2 * B]); ar += 3 * B; }
                }
                k.wd = k.wd + cross(k.w, wj);
                if (ar) k.wd = k.wd + k.R * v3(ar[0], ar[B], ar[2 * B]);
            }
            k.w = k.w + wj;
        }
        return;
    }
    const bool aligned = kind <= 3 || (kind >= FR_PX && kind < FR_PAXIS);
    const int c = kind <= 3 ? kind - 1 : kind - FR_PX;
    const V3<T> a = aligned ? v3(T(c == 0), T(c == 1), T(c == 2)) : v3((T)d[12], (T)d[13], (T)d[14]);
    const V3<T> z = k.R * a;      // (the joint's own motion leaves its axis where it is)
    if (kind >= FR_PX)
    {
        const V3<T> o2 = qr[0] * z;
        k.p = k.p + o2;
        if (moving)
        {
            const V3<T> wo = cross(k.w, o2);
            if (ACC)
            {
                k.pdd = k.pdd + cross(k.wd, o2) + cross(k.w, wo) + (T(2) * vr[0]) * cross(k.w, z);
                if (ar) k.pdd = k.pdd + ar[0] * z;
            }
            k.pd = k.pd + wo + vr[0] * z;
        }
        return;
    }
    T sn, cs;
    if (kind == SEG_UNBOUNDED) { cs = qr[0]; sn = qr[B]; }
    else sincos_(qr[0], &sn, &cs);
    k.R = k.R * (kind <= 3 ? rot_axis<T>(c, cs, sn) : rot_rodrigues<T>(a, cs, sn));
    if (moving)
    {
        if (ACC)
        {
            k.wd = k.wd + vr[0] * cross(k.w, z);
            if (ar) k.wd = k.wd + ar[0] * z;
        }
        k.w = k.w + vr[0] * z;
    }
}

// Pose and velocity of every frame of the plan for one lane.  q `[nq][B]`; v `[nv][B]` (read only when `vel` is given);
// model_lane `[13 * njoints][B]` or null: the translation of every joint placement is then the lane's own
// (rows 13 j + 10 .. 13 j + 12) instead of the plan's.  pose, pose_prev `[7][K][B]`; rpy `[3][K][B]`; vel `[6][K][B]`
// (linear, angular: LOCAL_WORLD_ALIGNED as (pdot, omega), any other mode as (R^T pdot, R^T omega)).  Every output may be null.
template<class T>
JM_DEV void frame_kinematics_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, const T * __restrict__ q,
                                  const T * __restrict__ v, const T * __restrict__ model_lane, T * __restrict__ pose,
                                  T * __restrict__ pose_prev, T * __restrict__ rpy, T * __restrict__ vel, long long B, long long lane)
{
    const int K = it[0], si = it[1];
    const long long KB = (long long)K * B;
    const bool moving = vel != nullptr;
    for (int f = 0; f < K; ++f)
    {
        const int s0 = it[2 + 3 * f], s1 = s0 + it[3 + 3 * f], mode = it[4 + 3 * f];
        FrameWalk<T> k = frame_walk_start<T>();
        for (int s = s0; s < s1; ++s)
            frame_walk_segment<T, false>(k, s == s0, dt + (long long)s * FR_SEG_DOUBLES, it + si + FR_SEG_INTS * s, q, v, nullptr,
                                         model_lane, moving, B, lane);
        const M3<T> & R = k.R;
        const V3<T> & p = k.p, & w = k.w, & pd = k.pd;
        const long long o = (long long)f * B + lane;
        const Quat<T> e = matrix_to_quat(R);
        if (pose)
        {
            pose[o] = p.x; pose[KB + o] = p.y; pose[2 * KB + o] = p.z;
            quat_store(pose + 3 * KB, KB, o, e);
        }
        if (pose_prev)
        {
            pose_prev[o] = p.x; pose_prev[KB + o] = p.y; pose_prev[2 * KB + o] = p.z;
            quat_store(pose_prev + 3 * KB, KB, o, e);
        }
        if (rpy) quat_store_rpy(rpy, KB, o, e);
        if (moving)
        {
            const V3<T> l = mode == FR_LOCAL_WORLD_ALIGNED ? pd : tmul(R, pd);
            const V3<T> g = mode == FR_LOCAL_WORLD_ALIGNED ? w : tmul(R, w);
            vel[o] = l.x; vel[KB + o] = l.y; vel[2 * KB + o] = l.z;
            vel[3 * KB + o] = g.x; vel[4 * KB + o] = g.y; vel[5 * KB + o] = g.z;
        }
    }
}

// ---- the step average.  The reference clamps its divisions with `np.finfo(np.float64).tiny` and powers of it; the constant
// of the kernel's own type stands here (a float64 `tiny` is zero in float32, and a lane at rest would divide 0 by 0).  The
// float32 root is rounded up so that its square stays a normal number.
template<class T> struct FrameTiny;
template<> struct FrameTiny<double>
{
    static constexpr double tiny = 2.2250738585072014e-308, root = 1.4916681462400413e-154, pow23 = 7.91096787527241e-206;
};
template<> struct FrameTiny<float>
{
    static constexpr float tiny = 1.17549435e-38f, root = 1.0842023e-19f, pow23 = 5.169879e-26f;
};

// a product kept as a value of its own under -ffp-contract=fast (`tilt_product` of jm_rotation.h): a difference of two
// equal products must be zero, which a product fused into the subtraction does not give
template<class T> JM_DEV T frame_product(T x) { return tilt_product<TILT_ROUNDED>(x); }

// `quat_multiply` (utils/math.py:611-622) with every product rounded and the four products of a component summed in
// pairs that cancel -- (w_l v_r + v_l w_r) + (v_l x v_r) -- where the reference sums them left to right: conj(q) * q then has
// an exactly zero vector part, which the reference's own order does not give (a few 1e-18).
template<class T> JM_DEV Quat<T> frame_quat_mul(const Quat<T> & l, const Quat<T> & r, T sl, T sr)
{
    const T lw = sl * l.w, rw = sr * r.w;
    return {(frame_product(lw * r.x) + frame_product(l.x * rw)) + (frame_product(l.y * r.z) - frame_product(l.z * r.y)),
            (frame_product(lw * r.y) + frame_product(l.y * rw)) + (frame_product(l.z * r.x) - frame_product(l.x * r.z)),
            (frame_product(lw * r.z) + frame_product(l.z * rw)) + (frame_product(l.x * r.y) - frame_product(l.y * r.x)),
            frame_product(lw * rw) - frame_product(l.x * r.x) - frame_product(l.y * r.y) - frame_product(l.z * r.z)};
}

// `quat_apply` (utils/math.py:687-705); s = -1 applies the conjugate
template<class T> JM_DEV V3<T> frame_quat_apply(const Quat<T> & q, V3<T> u, T s)
{
    const T xx = q.x * q.x, xy = q.x * q.y, xz = q.x * q.z, xw = q.x * q.w;
    const T yy = q.y * q.y, yz = q.y * q.z, yw = q.y * q.w, zz = q.z * q.z, zw = q.z * q.w, ww = q.w * q.w;
    return {u.x * (xx + ww - yy - zz) + u.y * (T(2) * xy - T(2) * s * zw) + u.z * (T(2) * xz + T(2) * s * yw),
            u.x * (T(2) * s * zw + T(2) * xy) + u.y * (ww - xx + yy - zz) + u.z * (-T(2) * s * xw + T(2) * yz),
            u.x * (-T(2) * s * yw + T(2) * xz) + u.y * (T(2) * s * xw + T(2) * yz) + u.z * (ww - xx - yy + zz)};
}

template<class T> JM_DEV T frame_sign(T x) { return x > T(0) ? T(1) : (x < T(0) ? T(-1) : T(0)); }

// `remove_yaw_from_quat` (utils/math.py:1176-1194).  Every product is rounded on its own, as the reference evaluates it: the
// half angles come from `1 - cos`, where one ulp of the cosine is amplified by 1 / (4 sin(angle / 2)) -- at 2 mrad of roll
// a product fused into the sum in front of it moved the result by 2.4e-14, and an odometry velocity of 12 m/s with it by
// 5e-13, against a bar of 1e-13.
template<class T> JM_DEV Quat<T> frame_remove_yaw(const Quat<T> & q)
{
    const T xx = frame_product(q.x * q.x), xz = frame_product(q.x * q.z), xw = frame_product(q.x * q.w);
    const T yy = frame_product(q.y * q.y), yz = frame_product(q.y * q.z), yw = frame_product(q.y * q.w);
    T cos_roll = T(1) - T(2) * (xx + yy);
    const T sin_roll = T(2) * (xw + yz);
    cos_roll /= sqrt_(frame_product(cos_roll * cos_roll) + frame_product(sin_roll * sin_roll));
    const T cos_roll_2 = sqrt_(T(0.5) * (T(1) + cos_roll));
    const T sin_roll_2 = frame_sign(sin_roll) * sqrt_(T(0.5) * (T(1) - cos_roll));
    const T sin_pitch = T(2) * (yw - xz);
    const T cos_pitch = sqrt_(T(1) - frame_product(sin_pitch * sin_pitch));
    const T cos_pitch_2 = sqrt_(T(0.5) * (T(1) + cos_pitch));
    const T sin_pitch_2 = frame_sign(sin_pitch) * sqrt_(T(0.5) * (T(1) - cos_pitch));
    return {sin_roll_2 * cos_pitch_2, cos_roll_2 * sin_pitch_2, -sin_roll_2 * sin_pitch_2, cos_roll_2 * cos_pitch_2};
}

// The step average of every frame of the plan for one lane.  pose_prev, pose, pose_mean `[7][K][B]`; v_avg `[6][K][B]`;
// quat_no_yaw `[4][K][B]`; the three outputs may be null.  Last, `pose` becomes `pose_prev`.
template<class T>
JM_DEV void frame_average_lane(const int32_t * __restrict__ it, T * __restrict__ pose_prev, const T * __restrict__ pose, T inv_step_dt,
                               T * __restrict__ v_avg, T * __restrict__ pose_mean, T * __restrict__ quat_no_yaw, long long B,
                               long long lane)
{
    const int K = it[0];
    const long long KB = (long long)K * B;
    for (int f = 0; f < K; ++f)
    {
        const int mode = it[4 + 3 * f];
        const long long o = (long long)f * B + lane;
        const V3<T> x0 = v3(pose_prev[o], pose_prev[KB + o], pose_prev[2 * KB + o]);
        const V3<T> x1 = v3(pose[o], pose[KB + o], pose[2 * KB + o]);
        const Quat<T> q0 = quat_load(pose_prev + 3 * KB, f, KB, B, lane), q1 = quat_load(pose + 3 * KB, f, KB, B, lane);
        // `xyzquat_difference` (:1033-1042): the residual pose in the frame of the previous one
        const V3<T> pos = frame_quat_apply(q0, x1 - x0, T(-1));
        const Quat<T> qd = frame_quat_mul(q0, q1, T(-1), T(1));
        // `log3` (:766-770)
        const T sin_2 = sqrt_(qd.x * qd.x + qd.y * qd.y + qd.z * qd.z);
        T theta = T(2) * atan2_(sin_2, qd.w < T(0) ? -qd.w : qd.w);
        const T inv_sinc = theta / fmax_(sin_2, FrameTiny<T>::tiny), sg = frame_sign(qd.w);
        const V3<T> ang = v3(inv_sinc * qd.x * sg, inv_sinc * qd.y * sg, inv_sinc * qd.z * sg);
        // `log6` (:876-890)
        V3<T> lin;
        {
            const T eps = FrameTiny<T>::root;
            const T cot_2 = (qd.w < T(0) ? -qd.w : qd.w) / fmax_(sin_2, eps);
            theta = fmax_(theta, eps);
            const T beta = T(1) / (theta * theta) - T(0.5) * cot_2 / theta;
            const V3<T> wxv = cross(ang, pos), w2xv = cross(ang, wxv);
            lin = v3(pos.x - T(0.5) * wxv.x + beta * w2xv.x, pos.y - T(0.5) * wxv.y + beta * w2xv.y,
                     pos.z - T(0.5) * wxv.z + beta * w2xv.z);
        }
        // `integrate(pose, -0.5 * diff)`: `exp6` (:929-950) with `exp3` (:815-821), composed on the right of the pose
        V3<T> xm;
        Quat<T> qm;
        {
            const V3<T> vl = T(-0.5) * lin, va = T(-0.5) * ang;
            const T sum_sq = va.x * va.x + va.y * va.y + va.z * va.z;
            const T theta_sq = fmax_(sum_sq, FrameTiny<T>::pow23), th = sqrt_(theta_sq);
            T sn, cs;
            sincos_(th, &sn, &cs);
            const T alpha_wxv = (T(1) - cs) / theta_sq, alpha_w2 = (th - sn) / theta_sq / th;
            const V3<T> wxv = cross(va, vl), w2xv = cross(va, wxv);
            const V3<T> te = v3(vl.x + alpha_wxv * wxv.x + alpha_w2 * w2xv.x, vl.y + alpha_wxv * wxv.y + alpha_w2 * w2xv.y,
                                vl.z + alpha_wxv * wxv.z + alpha_w2 * w2xv.z);
            const T th3 = sqrt_(sum_sq), den = fmax_(th3, FrameTiny<T>::tiny);
            T sh, ch;
            sincos_(T(0.5) * th3, &sh, &ch);
            const Quat<T> qe = {sh * (va.x / den), sh * (va.y / den), sh * (va.z / den), ch};
            xm = x1 + frame_quat_apply(q1, te, T(1));
            qm = frame_quat_mul(q1, qe, T(1), T(1));
        }
        const Quat<T> qny = frame_remove_yaw(qm);
        if (pose_mean)
        {
            pose_mean[o] = xm.x; pose_mean[KB + o] = xm.y; pose_mean[2 * KB + o] = xm.z;
            quat_store(pose_mean + 3 * KB, KB, o, qm);
        }
        if (quat_no_yaw) quat_store(quat_no_yaw, KB, o, qny);
        if (v_avg)
        {
            // (generic.py:1524-1532, locomotion.py:284-286)
            V3<T> l = inv_step_dt * lin, g = inv_step_dt * ang;
            if (mode != FR_LOCAL)
            {
                const Quat<T> & r = mode == FR_ODOMETRY ? qny : qm;
                l = frame_quat_apply(r, l, T(1));
                g = frame_quat_apply(r, g, T(1));
            }
            v_avg[o] = l.x; v_avg[KB + o] = l.y; v_avg[2 * KB + o] = l.z;
            v_avg[3 * KB + o] = g.x; v_avg[4 * KB + o] = g.y; v_avg[5 * KB + o] = g.z;
        }
        pose_prev[o] = x1.x; pose_prev[KB + o] = x1.y; pose_prev[2 * KB + o] = x1.z;
        quat_store(pose_prev + 3 * KB, KB, o, q1);
    }
}

#ifndef JM_HOST_EMU
struct FramesArgs
{
    const int32_t * it;
    const double * dt;
};
template<class T>
__global__ void __launch_bounds__(256) k_frame_kinematics(const FramesArgs p, const T * __restrict__ q, const T * __restrict__ v,
                                                           const T * __restrict__ model_lane, const uint8_t * __restrict__ lane_mask,
                                                           T * __restrict__ pose, T * __restrict__ pose_prev, T * __restrict__ rpy,
                                                           T * __restrict__ vel, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (lane_mask && !lane_mask[lane]) return;
    frame_kinematics_lane<T>(p.it, p.dt, q, v, model_lane, pose, pose_prev, rpy, vel, B, lane);
}

template<class T>
__global__ void __launch_bounds__(256) k_frame_average(const FramesArgs p, T * __restrict__ pose_prev, const T * __restrict__ pose,
                                                        double inv_step_dt, T * __restrict__ v_avg, T * __restrict__ pose_mean,
                                                        T * __restrict__ quat_no_yaw, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    frame_average_lane<T>(p.it, pose_prev, pose, (T)inv_step_dt, v_avg, pose_mean, quat_no_yaw, B, lane);
}
#endif
}  // namespace jm
