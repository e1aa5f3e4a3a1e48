// jm_locomotion.h -- the balance quantities of the reference's locomotion layer as one batched HIP kernel: centre of mass,
// odometry pose, zero-moment point, capture point, angular momentum of the base, normalised contact forces, vertical foot
// forces, and the scalars the momentum / friction rewards and the flying / impact terminations read.  Every lane is one
// environment, arrays are `[rows][B]` like the physics state.  Everything is read from what a step left in device memory:
// the `centroidal` rows, the root rows of `q`, the contact multipliers and flags of the constraint state and three tensors
// of the frame kinematics block (jm_frames.h).
//
// Reference (python/gym_jiminy/common/gym_jiminy/common, restated per lane, operation for operation):
//   CenterOfMass.refresh                          quantities/locomotion.py:814-887 (vcom: core/src/engine/engine.cc:896)
//   BaseOdometryPose                              quantities/locomotion.py:158-219, with `quat_to_yaw_cos_sin` / `quat_to_yaw`
//                                                 (utils/math.py:95-141) on the root quaternion of `q`
//   translate_position_odom                       quantities/locomotion.py:891-910
//   ZeroMomentPoint.refresh                       quantities/locomotion.py:996-1017
//   CapturePoint.refresh                          quantities/locomotion.py:1114-1124
//   AverageBaseMomentum.refresh                   quantities/locomotion.py:404-412
//   normalize_spatial_forces                      quantities/locomotion.py:1128-1155
//   normalize_vertical_forces                     quantities/locomotion.py:1272-1312 (flat ground: every vertical transform is e_z)
//   min_depth                                     compositions/locomotion.py:450-473 (flat ground: heights 0, normals e_z)
//   radial_basis_function, CUTOFF_ESP             compositions/mixin.py:17-66
// On a height map (`locomotion_lane<T, true>` with `ground_h` bound; jm_ground.h):
//   MultiFootNormalizedForceVertical.refresh      quantities/locomotion.py:1468-1481: the vertical transform of a contact is the
//                                                 third row of its constraint's `local_rotation` = [t0 t1 n]
//                                                 (FrameConstraint::setNormal, frame_constraint.cc:62-68)
//   _MultiContactMinGroundDistance.refresh        compositions/locomotion.py:527-540: height and normal of the ground under
//                                                 every contact point, min((z - height) * normal_z)
//
// All lanes interpret the same plan tables: their reads are indexed by loop counters only and become scalar loads.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "jm_frames.h"
#include "jm_ground.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_contacts, n_feet, zmp_frame, dcm_frame, n_frames, root_column, njoints,
// n_contacts x (foot, frame column)]; `dt` (float64) = [|gravity_z|, omega, mass of the robot, root inertia xx xy xz yy yz zz].
constexpr int LOCO_HEAD_INTS = 7;
constexpr int LOCO_GRAVITY = 0, LOCO_OMEGA = 1, LOCO_MASS = 2, LOCO_INERTIA = 3, LOCO_DOUBLES = 9;
constexpr int LOCO_MAX_CONTACTS = 256;
constexpr double LOCO_CUTOFF_ESP = 1.0e-2;           // (compositions/mixin.py:17)
constexpr double LOCO_ZMP_EPS = 1.1920928955078125e-07;  // np.finfo(np.float32).eps, whatever the kernel's scalar type (:1003)
// rows of the `scalars` output
constexpr int LOCO_FORCE_VERTICAL_MAX = 0, LOCO_GROUND_DISTANCE_MIN = 1, LOCO_REWARD_MOMENTUM = 2, LOCO_REWARD_FRICTION = 3;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool locomotion_pack(const jm_locomotion_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_locomotion_plan_create: ";
    if (!d) { why = who + "null description"; return false; }
    if (!d->body_mass || !d->root_inertia || !d->contact_foot || !d->contact_column)
    { why = who + "null array in the description"; return false; }
    if (d->njoints < 2) { why = who + "bad sizes: a floating base needs njoints >= 2"; return false; }
    if (d->n_contacts < 1 || d->n_contacts > LOCO_MAX_CONTACTS || d->n_feet < 1 || d->n_feet > d->n_contacts || d->n_frames < 1)
    { why = who + "bad sizes (1 <= n_feet <= n_contacts <= " + std::to_string(LOCO_MAX_CONTACTS) + ", n_frames >= 1)"; return false; }
    double mass = 0.0;
    for (int j = 0; j < d->njoints; ++j)
    {
        if (!std::isfinite(d->body_mass[j]) || d->body_mass[j] < 0.0)
        { why = who + "body_mass[" + std::to_string(j) + "] is negative or not finite"; return false; }
        if (j >= 1) mass += d->body_mass[j];       // (joint 0 is the universe; the order of the per-lane sum)
    }
    if (!(mass > 0.0)) { why = who + "the robot has no mass"; return false; }
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(d->root_inertia[k])) { why = who + "root_inertia is not finite"; return false; }
    if (!std::isfinite(d->gravity) || !(d->gravity > 0.0)) { why = who + "gravity must be the positive norm |gravity_z|"; return false; }
    if (!std::isfinite(d->omega) || !(d->omega > 0.0)) { why = who + "omega must be positive and finite"; return false; }
    for (int m : {d->zmp_frame, d->dcm_frame})
        if (m != FR_LOCAL && m != FR_LOCAL_WORLD_ALIGNED)
        { why = who + "Reference frame must be either LOCAL (0) or LOCAL_WORLD_ALIGNED (1)."; return false; }
    if (d->root_column < 0 || d->root_column >= d->n_frames)
    { why = who + "root_column " + std::to_string(d->root_column) + " out of range [0, " + std::to_string(d->n_frames) + ")"; return false; }
    std::vector<int> first(d->n_feet, -1), last(d->n_feet, -1);
    for (int c = 0; c < d->n_contacts; ++c)
    {
        const int f = d->contact_foot[c], col = d->contact_column[c];
        if (f < -1 || f >= d->n_feet)
        { why = who + "contact_foot[" + std::to_string(c) + "] = " + std::to_string(f) + " out of range [-1, " + std::to_string(d->n_feet) + ")"; return false; }
        if (col < 0 || col >= d->n_frames)
        { why = who + "contact_column[" + std::to_string(c) + "] = " + std::to_string(col) + " out of range [0, " + std::to_string(d->n_frames) + ")"; return false; }
        if (f >= 0)
        {
            if (first[f] < 0) first[f] = c;
            else if (last[f] != c - 1)
            { why = who + "Contact frames associated with identical parent body must be consecutive."; return false; }   // (:1440-1449)
            last[f] = c;
        }
    }
    for (int f = 0; f < d->n_feet; ++f)
        if (first[f] < 0) { why = who + "foot " + std::to_string(f) + " has no contact"; return false; }
    it = {d->n_contacts, d->n_feet, d->zmp_frame, d->dcm_frame, d->n_frames, d->root_column, d->njoints};
    for (int c = 0; c < d->n_contacts; ++c) { it.push_back(d->contact_foot[c]); it.push_back(d->contact_column[c]); }
    dt = {d->gravity, d->omega, mass};
    dt.insert(dt.end(), d->root_inertia, d->root_inertia + 6);
    return true;
}

// Validate the ground description of one launch (`jm_block_locomotion_ground`); null or without heights: flat ground.
inline bool locomotion_ground_check(const jm_locomotion_ground * g, const jm_locomotion_io * io, std::string & why)
{
    const std::string who = "jm_block_locomotion_ground: ";
    if (!g || !g->heights) return true;
    if (g->nx < 2 || g->ny < 2) { why = who + "the height map needs at least 2 x 2 samples"; return false; }
    if (!std::isfinite(g->x0) || !std::isfinite(g->y0)) { why = who + "the origin of the height map is not finite"; return false; }
    if (!std::isfinite(g->dx) || !std::isfinite(g->dy) || !(g->dx > 0.0) || !(g->dy > 0.0))
    { why = who + "the spacings of the height map must be positive and finite"; return false; }
    if (!io->pose) { why = who + "the queries of the height map read `pose`"; return false; }
    return true;
}

// the inputs and outputs of one launch (device pointers of the kernel's scalar type but `con_flags`); every one may be null
template<class T> struct LocoIO
{
    const T * centroidal;      // [15][B] com(3), hg(6), dhg(6)
    const T * q_root;          // [7][B] the root pose rows of q: position, quaternion xyzw
    const T * model_lane;      // [13 njoints][B]
    const T * con_lambda;      // [4 n_contacts][B] the contact multipliers
    const int32_t * con_flags; // [n_contacts][B] bit 0: enabled
    const T * v_avg;           // [6][K][B] step-average velocity of the frames block (root column: LOCAL)
    const T * quat_no_yaw;     // [4][K][B]
    const T * pose;            // [7][K][B]
    const uint8_t * lane_mask; // [B]
    T * com; T * vcom; T * odom_pose; T * zmp; T * dcm; T * h_angular;
    T * contact_force_rel;     // [6][n_contacts][B]
    T * foot_force_vertical;   // [n_feet][B]
    T * scalars;               // [4][B]
    // the ground under the contact points (`locomotion_lane<T, true>` only; null `ground_h`: flat ground): the height map in
    // the fields of `ground_profile` (jm_ground.h), the lanes' offsets of its queries and what it gives under every contact
    const T * ground_h = nullptr;       // [ground_ny][ground_nx]
    int ground_nx = 0, ground_ny = 0;
    T ground_x0 = T(0), ground_y0 = T(0), ground_dx = T(1), ground_dy = T(1);
    const T * ground_off = nullptr;     // [2][B] or null
    T * contact_ground = nullptr;       // [4][n_contacts][B] height, unit normal
};

JM_DEV double loco_pow(double x, double y) { return ::pow(x, y); }
JM_DEV float loco_pow(float x, float y) { return ::powf(x, y); }

// `translate_position_odom` (quantities/locomotion.py:904-910)
template<class T> JM_DEV void loco_translate_odom(T & x, T & y, T ref_x, T ref_y, T yaw)
{
    const T rx = x - ref_x, ry = y - ref_y;
    T sn, cs;
    sincos_(yaw, &sn, &cs);
    x = cs * rx + sn * ry;
    y = -sn * rx + cs * ry;
}

// `radial_basis_function(error, cutoff, 2)` of the squared norm of the error (compositions/mixin.py:56-66)
template<class T> JM_DEV T loco_rbf(T sq_norm, T cutoff)
{
    return loco_pow(T(LOCO_CUTOFF_ESP), sq_norm / loco_pow(cutoff, T(2)));
}

// Height and unit normal of the ground under the frame of column `col` of `pose`, queried at the lane's offset; `z`: the
// world height of the frame
template<class T> JM_DEV void loco_ground_under(const LocoIO<T> & io, int col, long long KB, long long B, long long lane, T & z, T & h,
                                                V3<T> & n)
{
    const T * p = io.pose + (long long)col * B + lane;
    T x = p[0], y = p[KB];
    z = p[2 * KB];
    if (io.ground_off) { x += io.ground_off[lane]; y += io.ground_off[B + lane]; }
    ground_profile(io, x, y, h, n);
}

// `contact_ground` of the flat ground: height 0 and normal e_z under every contact point
template<class T> JM_DEV void loco_flat_contact_ground(T * contact_ground, int nc, long long B, long long lane)
{
    for (long long r = 0; r < 4LL * nc; ++r) contact_ground[r * B + lane] = r < 3LL * nc ? T(0) : T(1);
}

// All quantities of one lane.  A part whose inputs or output are null is skipped.  GND: on the height map of `io` where one
// is bound (its queries read `pose`); GND = false is the flat ground at compile time.
template<class T, bool GND = false>
JM_DEV void locomotion_lane(const int32_t * __restrict__ it, const double * __restrict__ dt, const LocoIO<T> & io, T momentum_cutoff,
                            T friction_cutoff, long long B, long long lane)
{
    const int nc = it[0], zmp_frame = it[2], dcm_frame = it[3], K = it[4], root = it[5], nj = it[6];
    const long long KB = (long long)K * B;
    const int32_t * con = it + LOCO_HEAD_INTS;
    bool ground = false;
    if constexpr (GND) ground = io.ground_h && io.pose;
    // mass of the robot (`pinocchio_data.mass[0]`) and its weight (:981-983)
    T mass = (T)dt[LOCO_MASS];
    if (io.model_lane)
    {
        mass = T(0);
        for (int j = 1; j < nj; ++j) mass += io.model_lane[(long long)j * MODEL_LANE_ROWS * B + lane];
    }
    const T weight = frame_product(mass * (T)dt[LOCO_GRAVITY]);     // (a value of its own, as the reference keeps it)

    // `BaseOdometryPose` (:211-219)
    T ox = T(0), oy = T(0), yaw = T(0);
    if (io.q_root)
    {
        const T * r = io.q_root + lane;
        ox = r[0]; oy = r[B];
        const T qx = r[3 * B], qy = r[4 * B], qz = r[5 * B], qw = r[6 * B];
        const T q_xy = qy * qx, q_yy = qy * qy, q_zz = qz * qz, q_zw = qz * qw;    // (utils/math.py:103-105)
        yaw = atan2_(T(2) * (q_xy + q_zw), T(1) - T(2) * (q_yy + q_zz));
        if (io.odom_pose) { io.odom_pose[lane] = ox; io.odom_pose[B + lane] = oy; io.odom_pose[2 * B + lane] = yaw; }
    }
    if (io.centroidal)
    {
        const T * c = io.centroidal + lane;
        const T cx = c[0], cy = c[B], cz = c[2 * B];
        const T vx = c[3 * B] / mass, vy = c[4 * B] / mass, vz = c[5 * B] / mass;      // (engine.cc:896)
        if (io.com) { io.com[lane] = cx; io.com[B + lane] = cy; io.com[2 * B + lane] = cz; }
        if (io.vcom) { io.vcom[lane] = vx; io.vcom[B + lane] = vy; io.vcom[2 * B + lane] = vz; }
        if (io.zmp && (io.q_root || zmp_frame != FR_LOCAL))
        {
            // (:998-1015)
            const T dl_x = c[9 * B], dl_y = c[10 * B], dl_z = c[11 * B], da_x = c[12 * B], da_y = c[13 * B];
            const T f_z = dl_z + weight;
            T zx, zy;
            if (fabs_(f_z) < T(LOCO_ZMP_EPS)) zx = zy = T(NAN);
            else
            {
                const T ratio = weight / f_z;
                zx = cx * ratio; zy = cy * ratio;
                zx -= (da_y + dl_x * cz) / f_z;
                zy += (da_x - dl_y * cz) / f_z;
                if (zmp_frame == FR_LOCAL) loco_translate_odom(zx, zy, ox, oy, yaw);
            }
            io.zmp[lane] = zx; io.zmp[B + lane] = zy;
        }
        if (io.dcm && (io.q_root || dcm_frame != FR_LOCAL))
        {
            // (:1116-1122)
            const T omega = (T)dt[LOCO_OMEGA];
            T dx = cx + vx / omega, dy = cy + vy / omega;
            if (dcm_frame == FR_LOCAL) loco_translate_odom(dx, dy, ox, oy, yaw);
            io.dcm[lane] = dx; io.dcm[B + lane] = dy;
        }
    }

    // `AverageBaseMomentum` (:405-410)
    if (io.v_avg && io.quat_no_yaw && (io.h_angular || (io.scalars && momentum_cutoff > T(0))))
    {
        T ixx = (T)dt[LOCO_INERTIA], ixy = (T)dt[LOCO_INERTIA + 1], ixz = (T)dt[LOCO_INERTIA + 2];
        T iyy = (T)dt[LOCO_INERTIA + 3], iyz = (T)dt[LOCO_INERTIA + 4], izz = (T)dt[LOCO_INERTIA + 5];
        if (io.model_lane)
        {
            const T * ml = io.model_lane + ((long long)MODEL_LANE_ROWS + 4) * B + lane;     // (joint 1, behind mass and com)
            ixx = ml[0]; ixy = ml[B]; ixz = ml[2 * B]; iyy = ml[3 * B]; iyz = ml[4 * B]; izz = ml[5 * B];
        }
        const long long o = (long long)root * B + lane;
        const V3<T> w = v3(io.v_avg[3 * KB + o], io.v_avg[4 * KB + o], io.v_avg[5 * KB + o]);
        const M3<T> I = {ixx, ixy, ixz, ixy, iyy, iyz, ixz, iyz, izz};
        const V3<T> h = frame_quat_apply(quat_load(io.quat_no_yaw, root, KB, B, lane), I * w, T(1));
        if (io.h_angular) { io.h_angular[lane] = h.x; io.h_angular[B + lane] = h.y; io.h_angular[2 * B + lane] = h.z; }
        if (io.scalars && momentum_cutoff > T(0))
            io.scalars[(long long)LOCO_REWARD_MOMENTUM * B + lane] = loco_rbf(h.x * h.x + h.y * h.y + h.z * h.z, momentum_cutoff);
    }

    // `normalize_spatial_forces` (:1147-1155), `normalize_vertical_forces` (:1300-1312); a contact whose constraint is
    // disabled carries no force, whatever its multiplier rows hold
    if (io.con_lambda && io.con_flags)
    {
        const long long NB = (long long)nc * B;
        T f_max = T(0), sq_tangential = T(0), foot_sum = T(0);
        int foot = -1;
        for (int c = 0; c < nc; ++c)
        {
            const bool on = (io.con_flags[(long long)c * B + lane] & 1) != 0;
            const T * l = io.con_lambda + (long long)(4 * c) * B + lane;
            const T lx = on ? l[0] : T(0), ly = on ? l[B] : T(0), lz = on ? l[2 * B] : T(0), lt = on ? l[3 * B] : T(0);
            const T fx = lx / weight, fy = ly / weight, fz = lz / weight;
            if (io.contact_force_rel)
            {
                T * o = io.contact_force_rel + (long long)c * B + lane;
                o[0] = fx; o[NB] = fy; o[2 * NB] = fz; o[3 * NB] = T(0); o[4 * NB] = T(0); o[5 * NB] = lt / weight;
            }
            f_max = c == 0 ? fz : fmax_(f_max, fz);
            sq_tangential += fx * fx + fy * fy;
            // (the contacts of a foot are consecutive: the plan was checked for it)
            const int f = con[2 * c];
            if (f != foot)
            {
                if (foot >= 0 && io.foot_force_vertical) io.foot_force_vertical[(long long)foot * B + lane] = foot_sum / weight;
                foot = f;
                foot_sum = T(0);
            }
            if constexpr (GND)
            {
                // the world vertical force: the third row of [t0 t1 n] on the local multipliers (:1308)
                T vz = lz;
                if (ground)
                {
                    T z, h;
                    V3<T> n, t0, t1;
                    loco_ground_under(io, con[2 * c + 1], KB, B, lane, z, h, n);
                    ground_tangents(n, t0, t1);
                    vz = t0.z * lx + t1.z * ly + n.z * lz;
                }
                foot_sum += vz;
            }
            else foot_sum += lz;
        }
        if (foot >= 0 && io.foot_force_vertical) io.foot_force_vertical[(long long)foot * B + lane] = foot_sum / weight;
        if (io.scalars)
        {
            io.scalars[(long long)LOCO_FORCE_VERTICAL_MAX * B + lane] = f_max;
            if (friction_cutoff > T(0)) io.scalars[(long long)LOCO_REWARD_FRICTION * B + lane] = loco_rbf(sq_tangential, friction_cutoff);
        }
    }

    // `min_depth` on the height map: (z - height) * normal_z of the ground under every contact frame (:472)
    if constexpr (GND)
        if (ground && (io.scalars || io.contact_ground))
        {
            const long long NB = (long long)nc * B;
            T d_min = T(0);
            for (int c = 0; c < nc; ++c)
            {
                T z, h;
                V3<T> n;
                loco_ground_under(io, con[2 * c + 1], KB, B, lane, z, h, n);
                if (io.contact_ground)
                {
                    T * o = io.contact_ground + (long long)c * B + lane;
                    o[0] = h; o[NB] = n.x; o[2 * NB] = n.y; o[3 * NB] = n.z;
                }
                const T d = (z - h) * n.z;
                d_min = c == 0 ? d : fmin_(d_min, d);
            }
            if (io.scalars) io.scalars[(long long)LOCO_GROUND_DISTANCE_MIN * B + lane] = d_min;
            return;
        }
    if constexpr (GND)
        if (io.contact_ground) loco_flat_contact_ground(io.contact_ground, nc, B, lane);       // (no map bound)
    // `min_depth` on flat ground: the lowest contact frame
    if (io.pose && io.scalars)
    {
        T z_min = T(0);
        for (int c = 0; c < nc; ++c)
        {
            const T z = io.pose[2 * KB + (long long)con[2 * c + 1] * B + lane];
            z_min = c == 0 ? z : fmin_(z_min, z);
        }
        io.scalars[(long long)LOCO_GROUND_DISTANCE_MIN * B + lane] = z_min;
    }
}

#ifndef JM_HOST_EMU
template<class T, bool GND = false>
__global__ void __launch_bounds__(256) k_locomotion(const int32_t * __restrict__ it, const double * __restrict__ dt, const LocoIO<T> io,
                                                     double momentum_cutoff, double friction_cutoff, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    locomotion_lane<T, GND>(it, dt, io, (T)momentum_cutoff, (T)friction_cutoff, B, lane);
}

// `contact_ground` where no map is bound: next to a launch of `k_locomotion<T>`, whose outputs the flat ground's must equal
// bit for bit
template<class T>
__global__ void __launch_bounds__(256) k_locomotion_flat_ground(const int32_t * __restrict__ it, T * contact_ground,
                                                                 const uint8_t * __restrict__ lane_mask, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (lane_mask && !lane_mask[lane]) return;
    loco_flat_contact_ground(contact_ground, it[0], B, lane);
}
#endif
}  // namespace jm
