// jm_footposes.h -- the foot pose quantities of the reference's locomotion layer as one batched HIP kernel: the mean pose of
// the feet, its odometry pose, the pose of every foot but the last relative to the mean, and the tracking error and the two
// tracking rewards against a caller-supplied reference of the relative poses.  Every lane is one environment, arrays are
// `[rows][B]` like the physics state.  Everything is read from the `pose` tensor of the frame kinematics block (jm_frames.h).
//
// Reference (python/gym_jiminy/common/gym_jiminy/common, restated per lane, operation for operation):
//   position_average, quat_average_2d             quantities/generic.py:950-980
//   quat_interpolate_middle                       utils/math.py:1296-1331 (two feet; `np.sign(dot)`: a dot product of exactly 0
//                                                 gives quat1 / sqrt(2))
//   MultiFrameMeanXYZQuat.refresh                 quantities/generic.py:984-1062
//   MultiFootMeanXYZQuat                          quantities/locomotion.py:416-478
//   MultiFootMeanOdometryPose.refresh             quantities/locomotion.py:482-557, with `quat_to_yaw` (utils/math.py:95-141)
//   quat_to_matrix                                utils/math.py:214-248
//   translate_positions,
//   MultiFootRelativeXYZQuat.refresh              quantities/locomotion.py:683-810 (the last foot is dropped)
//   log3, quat_difference                         utils/math.py:724-774, :971-1005
//   TrackingQuantityReward                        compositions/generic.py:64-122
//   TrackingFootPositionsReward,
//   TrackingFootOrientationsReward                compositions/locomotion.py:146-214
//   radial_basis_function, CUTOFF_ESP             compositions/mixin.py:17-66 (`loco_rbf` of jm_locomotion.h)
//
// Deviations, all of them where the reference's text leaves the value open:
//   * Three feet or more: the reference takes the last eigenvector of `quat @ quat.T` from LAPACK (`np.linalg.eigh`), whose
//     sign is arbitrary.  Here the eigenvector comes from a cyclic Jacobi iteration and its sign is defined: the mean
//     quaternion has a non-negative dot product with the quaternion of the first foot (what the two-foot branch gives by
//     construction).  Nothing downstream depends on the sign: the yaw, `log3` and `quat_difference` are even in it and the
//     relative quaternions flip with it.
//   * `log3` clamps its division with `np.finfo(np.float64).tiny`; the constant of the kernel's own type stands here
//     (`FrameTiny` of jm_frames.h: a float64 `tiny` is zero in float32, and an exact zero error would divide 0 by 0).
//   * The products of the two quaternion products are rounded one by one and summed in cancelling pairs (`frame_quat_mul`
//     of jm_frames.h), so that a reference equal to the relative pose gives an error of exactly zero and a reward of one.
//   * One foot: there is no relative pose, the error is empty and both rewards are `pow(CUTOFF_ESP, 0)` = 1, reference or not.
//
// All lanes interpret the same plan table: its reads are indexed by loop counters only and become scalar loads.  A lane
// keeps no array: the 10 + 16 numbers of the eigen solve are named scalars, and the second pass over the feet reads their
// rows again (they are in cache) instead of indexing a private copy.
#pragma once
#include <string>
#include <vector>

#include "jm_locomotion.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_frames, n_feet, n_feet x pose column]; `dt` (float64) = [n_feet, the divisor of
// `position_average`].
constexpr int FOOT_HEAD_INTS = 2;
constexpr int FOOT_MAX_FEET = 64;
// Sweeps of the cyclic Jacobi iteration, fixed so that a lane's bits depend on its own inputs only.  The iteration converges
// quadratically once the off-diagonal entries are below the gaps: restated in numpy on 200 000 draws of 3 to 64 quaternions
// spread up to pi around a common one (relative gap of the two largest eigenvalues down to 0.005), the largest off-diagonal
// entry was 3e-4 after 4 sweeps, 1.2e-14 after 5 and below 1e-38 after 6, in float64 and in float32 alike; the eigenvector
// then lay within 2.7e-15 of LAPACK's at a gap of 0.1 or more (2.7e-14 at 0.005).
constexpr int FOOT_JACOBI_SWEEPS = 6;
// rows of the `scalars` output
constexpr int FOOT_REWARD_POSITIONS = 0, FOOT_REWARD_ORIENTATIONS = 1;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool footposes_pack(const jm_footposes_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_footposes_plan_create: ";
    if (!d) { why = who + "null description"; return false; }
    if (!d->foot_column) { why = who + "null array in the description"; return false; }
    if (d->n_frames < 1 || d->n_feet < 1 || d->n_feet > FOOT_MAX_FEET || d->n_feet > d->n_frames)
    { why = who + "bad sizes (1 <= n_feet <= " + std::to_string(FOOT_MAX_FEET) + ", n_feet <= n_frames)"; return false; }
    for (int f = 0; f < d->n_feet; ++f)
    {
        const int col = d->foot_column[f];
        if (col < 0 || col >= d->n_frames)
        { why = who + "foot_column[" + std::to_string(f) + "] = " + std::to_string(col) + " out of range [0, " + std::to_string(d->n_frames) + ")"; return false; }
        for (int g = 0; g < f; ++g)
            if (d->foot_column[g] == col)
            { why = who + "foot_column[" + std::to_string(f) + "] repeats the column of foot " + std::to_string(g); return false; }
    }
    it = {d->n_frames, d->n_feet};
    it.insert(it.end(), d->foot_column, d->foot_column + d->n_feet);
    dt = {(double)d->n_feet};
    return true;
}

// the inputs and outputs of one launch (device pointers of the kernel's scalar type); every one may be null
template<class T> struct FootIO
{
    const T * pose;            // [7][K][B] of the frame kinematics block
    const T * reference;       // [7][F - 1][B] reference of `relative_pose`
    const uint8_t * lane_mask; // [B]
    T * mean_pose;             // [7][B]
    T * mean_odom_pose;        // [3][B]
    T * relative_pose;         // [7][F - 1][B]
    T * tracking_error;        // [6][F - 1][B]
    T * scalars;               // [2][B]
};

// One rotation of the Jacobi iteration on a symmetric 4 x 4 matrix, in the plane (p, q): `r`, `s` are the two other indices
// and `v?p`, `v?q` the columns p, q of the accumulated rotations.  t = tan of the angle is the smaller root of
// t^2 + 2 t theta - 1 = 0 with theta = (a_qq - a_pp) / (2 a_pq): |theta| overflowing gives t = 0, and an off-diagonal
// entry below the smallest normal number is not divided by: the rotation is then the identity, and every update below is
// an exact no-op (x - 0 * y = x).
template<class T>
JM_DEV void foot_jacobi_rotate(T & app, T & aqq, T & apq, T & arp, T & arq, T & asp, T & asq, T & v0p, T & v0q, T & v1p, T & v1q,
                               T & v2p, T & v2q, T & v3p, T & v3q)
{
    const bool on = fabs_(apq) > FrameTiny<T>::tiny;
    const T theta = (aqq - app) / (T(2) * (on ? apq : T(1)));
    const T root = T(1) / (fabs_(theta) + sqrt_(theta * theta + T(1)));
    const T t = on ? (theta < T(0) ? -root : root) : T(0);
    const T c = T(1) / sqrt_(t * t + T(1)), s = t * c, tau = s / (T(1) + c);
    app -= t * apq;
    aqq += t * apq;
    apq = on ? T(0) : apq;
    T g, h;
    g = arp; h = arq; arp = g - s * (h + tau * g); arq = h + s * (g - tau * h);
    g = asp; h = asq; asp = g - s * (h + tau * g); asq = h + s * (g - tau * h);
    g = v0p; h = v0q; v0p = g - s * (h + tau * g); v0q = h + s * (g - tau * h);
    g = v1p; h = v1q; v1p = g - s * (h + tau * g); v1q = h + s * (g - tau * h);
    g = v2p; h = v2q; v2p = g - s * (h + tau * g); v2q = h + s * (g - tau * h);
    g = v3p; h = v3q; v3p = g - s * (h + tau * g); v3q = h + s * (g - tau * h);
}

// The unit eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix given by its ten distinct entries (index
// 0..3 = x, y, z, w), ≙ `np.linalg.eigh(quat @ quat.T)[1][..., -1]` (quantities/generic.py:979-980) up to its sign.
template<class T> JM_DEV Quat<T> foot_dominant_eigenvector(T a00, T a01, T a02, T a03, T a11, T a12, T a13, T a22, T a23, T a33)
{
    T v00 = T(1), v01 = T(0), v02 = T(0), v03 = T(0), v10 = T(0), v11 = T(1), v12 = T(0), v13 = T(0);
    T v20 = T(0), v21 = T(0), v22 = T(1), v23 = T(0), v30 = T(0), v31 = T(0), v32 = T(0), v33 = T(1);
    for (int sweep = 0; sweep < FOOT_JACOBI_SWEEPS; ++sweep)
    {
        foot_jacobi_rotate(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);
        foot_jacobi_rotate(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);
        foot_jacobi_rotate(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);
        foot_jacobi_rotate(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);
        foot_jacobi_rotate(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);
        foot_jacobi_rotate(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);
    }
    // the column of the largest diagonal entry, selected scalar by scalar (a select between whole columns is a select
    // between addresses, and the sixteen entries then go through scratch)
    const bool b1 = a11 > a00;
    const T d1 = b1 ? a11 : a00, x1 = b1 ? v01 : v00, y1 = b1 ? v11 : v10, z1 = b1 ? v21 : v20, w1 = b1 ? v31 : v30;
    const bool b2 = a22 > d1;
    const T d2 = b2 ? a22 : d1, x2 = b2 ? v02 : x1, y2 = b2 ? v12 : y1, z2 = b2 ? v22 : z1, w2 = b2 ? v32 : w1;
    const bool b3 = a33 > d2;
    const T x = b3 ? v03 : x2, y = b3 ? v13 : y2, z = b3 ? v23 : z2, w = b3 ? v33 : w2;
    // (the product of 6 x sweeps rotations is orthogonal up to their roundings: LAPACK returns unit vectors)
    const T n = sqrt_(x * x + y * y + z * z + w * w);
    return {x / n, y / n, z / n, w / n};
}

// `log3` (utils/math.py:766-770)
template<class T> JM_DEV V3<T> foot_log3(const Quat<T> & q)
{
    const T theta_sin_2 = sqrt_(q.x * q.x + q.y * q.y + q.z * q.z);
    const T theta = T(2) * atan2_(theta_sin_2, fabs_(q.w));
    const T inv_sinc = theta / fmax_(theta_sin_2, FrameTiny<T>::tiny);
    const T sign = frame_sign(q.w);
    return {inv_sinc * q.x * sign, inv_sinc * q.y * sign, inv_sinc * q.z * sign};
}

// All quantities of one lane.  A part whose inputs or output are null is skipped.
template<class T>
JM_DEV void footposes_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, const FootIO<T> & io, T position_cutoff,
                           T orientation_cutoff, long long B, long long lane)
{
    if (!io.pose) return;
    const int K = it[0], F = it[1];
    const long long KB = (long long)K * B, RB = (long long)(F - 1) * B;
    const int32_t * col = it + FOOT_HEAD_INTS;

    // `position_average` (quantities/generic.py:958) and the entries of `quat @ quat.T` (:979), summed in the order of the feet
    T sx = T(0), sy = T(0), sz = T(0);
    T a00 = T(0), a01 = T(0), a02 = T(0), a03 = T(0), a11 = T(0), a12 = T(0), a13 = T(0), a22 = T(0), a23 = T(0), a33 = T(0);
    Quat<T> first = {T(0), T(0), T(0), T(1)}, second = first;
    for (int f = 0; f < F; ++f)
    {
        const long long o = (long long)col[f] * B + lane;
        const T px = io.pose[o], py = io.pose[KB + o], pz = io.pose[2 * KB + o];
        const Quat<T> q = quat_load(io.pose + 3 * KB, col[f], KB, B, lane);
        sx = f == 0 ? px : sx + px; sy = f == 0 ? py : sy + py; sz = f == 0 ? pz : sz + pz;
        if (f == 0) first = q;
        if (f == 1) second = q;
        a00 += q.x * q.x; a01 += q.x * q.y; a02 += q.x * q.z; a03 += q.x * q.w;
        a11 += q.y * q.y; a12 += q.y * q.z; a13 += q.y * q.w;
        a22 += q.z * q.z; a23 += q.z * q.w; a33 += q.w * q.w;
    }
    const T n_feet = (T)dt[0];
    const T mx = sx / n_feet, my = sy / n_feet, mz = sz / n_feet;

    // `quat_average_2d` (:973-980)
    Quat<T> mean = first;
    if (F == 2)
    {
        // `quat_interpolate_middle` (utils/math.py:1325-1327)
        const T d = first.x * second.x + first.y * second.y + first.z * second.z + first.w * second.w;
        const T sign = frame_sign(d), den = sqrt_(T(2) * (T(1) + fabs_(d)));
        mean = {(first.x + sign * second.x) / den, (first.y + sign * second.y) / den, (first.z + sign * second.z) / den,
                (first.w + sign * second.w) / den};
    }
    else if (F >= 3)
    {
        mean = foot_dominant_eigenvector(a00, a01, a02, a03, a11, a12, a13, a22, a23, a33);
        // the defined sign: a non-negative dot product with the first foot's quaternion
        if (mean.x * first.x + mean.y * first.y + mean.z * first.z + mean.w * first.w < T(0))
            mean = {-mean.x, -mean.y, -mean.z, -mean.w};
    }
    if (io.mean_pose)
    {
        T * o = io.mean_pose + lane;
        o[0] = mx; o[B] = my; o[2 * B] = mz; o[3 * B] = mean.x; o[4 * B] = mean.y; o[5 * B] = mean.z; o[6 * B] = mean.w;
    }
    // `MultiFootMeanOdometryPose.refresh` (quantities/locomotion.py:549-557; `quat_to_yaw`, utils/math.py:103-104, :140-141)
    if (io.mean_odom_pose)
    {
        const T q_xy = mean.y * mean.x, q_yy = mean.y * mean.y, q_zz = mean.z * mean.z, q_zw = mean.z * mean.w;
        io.mean_odom_pose[lane] = mx;
        io.mean_odom_pose[B + lane] = my;
        io.mean_odom_pose[2 * B + lane] = atan2_(T(2) * (q_xy + q_zw), T(1) - T(2) * (q_yy + q_zz));
    }

    // `MultiFootRelativeXYZQuat.refresh` (:779-810) and the tracking error of every foot but the last
    const bool tracking = io.reference && (io.tracking_error || io.scalars);
    T sq_position = T(0), sq_orientation = T(0);
    if (F >= 2 && (io.relative_pose || tracking))
    {
        // `quat_to_matrix` (utils/math.py:233-244)
        const T q_xx = mean.x * mean.x, q_xy = mean.x * mean.y, q_xz = mean.x * mean.z, q_xw = mean.x * mean.w;
        const T q_yy = mean.y * mean.y, q_yz = mean.y * mean.z, q_yw = mean.y * mean.w;
        const T q_zz = mean.z * mean.z, q_zw = mean.z * mean.w;
        const M3<T> R = {T(1) - T(2) * (q_yy + q_zz), T(2) * (q_xy - q_zw), T(2) * (q_xz + q_yw),
                         T(2) * (q_xy + q_zw), T(1) - T(2) * (q_xx + q_zz), T(2) * (q_yz - q_xw),
                         T(2) * (q_xz - q_yw), T(2) * (q_yz + q_xw), T(1) - T(2) * (q_xx + q_yy)};
        for (int f = 0; f < F - 1; ++f)
        {
            const long long o = (long long)col[f] * B + lane, r = (long long)f * B + lane;
            // `translate_positions` (:698), `quat_multiply(..., is_left_conjugate=True)` (:805-808)
            const V3<T> p = tmul(R, v3(io.pose[o] - mx, io.pose[KB + o] - my, io.pose[2 * KB + o] - mz));
            const Quat<T> q = frame_quat_mul(mean, quat_load(io.pose + 3 * KB, col[f], KB, B, lane), T(-1), T(1));
            if (io.relative_pose)
            {
                io.relative_pose[r] = p.x; io.relative_pose[RB + r] = p.y; io.relative_pose[2 * RB + r] = p.z;
                quat_store(io.relative_pose + 3 * RB, RB, r, q);
            }
            if (tracking)
            {
                // `operator.sub` and `quat_difference` (utils/math.py:1002-1005) of `TrackingQuantityReward` (:116-120)
                const T ex = p.x - io.reference[r], ey = p.y - io.reference[RB + r], ez = p.z - io.reference[2 * RB + r];
                const V3<T> w = foot_log3(frame_quat_mul(q, quat_load(io.reference + 3 * RB, f, RB, B, lane), T(-1), T(1)));
                if (io.tracking_error)
                {
                    T * e = io.tracking_error + r;
                    e[0] = ex; e[RB] = ey; e[2 * RB] = ez; e[3 * RB] = w.x; e[4 * RB] = w.y; e[5 * RB] = w.z;
                }
                sq_position += ex * ex + ey * ey + ez * ez;
                sq_orientation += w.x * w.x + w.y * w.y + w.z * w.z;
            }
        }
    }
    // `radial_basis_function(error, cutoff, 2)` (compositions/mixin.py:56-66); one foot: the error is empty
    if (io.scalars && (io.reference || F == 1))
    {
        if (position_cutoff > T(0)) io.scalars[(long long)FOOT_REWARD_POSITIONS * B + lane] = loco_rbf(sq_position, position_cutoff);
        if (orientation_cutoff > T(0))
            io.scalars[(long long)FOOT_REWARD_ORIENTATIONS * B + lane] = loco_rbf(sq_orientation, orientation_cutoff);
    }
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_foot_poses(const int32_t * __restrict__ it, const double * __restrict__ dt, const FootIO<T> io,
                                                     double position_cutoff, double orientation_cutoff, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    footposes_lane<T>(it, dt, io, (T)position_cutoff, (T)orientation_cutoff, B, lane);
}
#endif
}  // namespace jm
