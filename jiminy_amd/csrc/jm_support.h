// jm_support.h -- the projected support polygon of the reference's toolbox as one batched HIP kernel: the 2D convex hull of
// every candidate contact point, its barycenter, the signed distance of the ZMP from its border (the stability margin) and the
// robustness reward on it.  Every lane is one environment, arrays are `[rows][B]` like the physics state.  The points are
// read from the `pose` tensor of the frame kinematics block (jm_frames.h), `odom_pose` and `zmp` from the locomotion
// quantities block (jm_locomotion.h).
//
// Reference (python/gym_jiminy/toolbox/gym_jiminy/toolbox, restated per lane, operation for operation):
//   compute_convex_hull_vertices                  math/qhull.py:52-123 (two stable sorts :71-72, `npoints <= 3` :75-77,
//                                                 Andrew's monotone chains :82-123)
//   compute_vectors_from_convex                   math/qhull.py:127-145
//   compute_distance_convex_to_point              math/qhull.py:183-224
//   ConvexHull2D.center, .get_distance_to_point   math/qhull.py:396-457 (the branch is on the number of POINTS)
//   ProjectedSupportPolygon.refresh               quantities/locomotion.py:146-160
//   StabilityMarginProjectedSupportPolygon.refresh  quantities/locomotion.py:228-239
//   sigmoid_normalization, MaximizeRobustness     compositions/locomotion.py:15-115
//   translate_position_odom                       common/quantities/locomotion.py:890-911 (of gym_jiminy/common)
//   CUTOFF_ESP                                    common/compositions/mixin.py:17 (`LOCO_CUTOFF_ESP` of jm_locomotion.h)
//
// Not built: `ProjectedSupportPolygon.initialize` (:83-144) prunes, once and on the host, the contact points that are not
// vertices of the 3D convex hull of their body (scipy's `ConvexHull`).  By the reference's own argument (:110-119) this is
// an optimisation that does not change the polygon.  Here every contact point of the plan is a candidate, in the model's
// contact order, so `vertex_index` counts in that order.
//
// The orientation predicates.  Each one compares two products, `a * b > c * d`, as the reference writes them, never the sign
// of their difference: the library is built with -ffp-contract=fast, which would fuse one product of `a * b - c * d` into
// the subtraction, and a comparison of two products has nothing to contract.  The predicate then has the bits numpy gives on
// the same inputs, and exact ties (duplicate points, collinear points, a query on an edge) fall as in the reference.  For the
// same reason the four products of `translate_position_odom` are rounded one by one (`frame_product` of jm_frames.h): a
// point is translated again wherever it is read, and has to come out with the same bits every time.
//
// Which form was built: REGISTERS.  A lane keeps no array.  The sorted order, the stack of each chain and the vertex list
// hold at most 16 indices of 4 bits: each is one 64-bit register, pushed and popped by shifts.  The coordinates of a point
// are read again from `pose` by its index whenever they are needed (at most 32 values per lane, which sit in cache); the two
// points on top of a chain's stack are kept in named scalars, so that only a pop reads memory.  The sort is a rank count:
// the plan table is read through loop counters only there (scalar loads); a chain reads the column of a popped-to point by
// a per-lane index, which is a gather from the plan in global memory, not a private array.
//
// Termination is structural.  Every loop counts to `n_points` (a plan constant) or to SUPPORT_MAX_POINTS, whatever the data
// holds, and the pops of a chain count down the length of its own stack.  The order of the rank count is total on every bit
// pattern: a NaN sorts behind every number and ties with another NaN (numpy's order), -0 ties with +0, and the index decides
// last, so the ranks are a permutation of 0 .. n_points - 1 and every index a lane ever forms is one of the plan's.  On NaN
// or infinite coordinates every predicate is false and every point is popped: such a lane ends with two vertices per chain
// and a margin that is NaN or arbitrary, and touches nothing of another lane.  The two chains of finite but nearly collinear
// points may, through rounding, keep more vertices than there are points; the vertex list stops at SUPPORT_MAX_POINTS.
#pragma once
#include <string>
#include <vector>

#include "jm_locomotion.h"
#include "../../include/jiminy_hip.h"

namespace jm
{
// ---- the packed plan: `it` (int32) = [n_frames, n_points, reference_frame, n_points x pose column]; `dt` is not read.
constexpr int SUPPORT_HEAD_INTS = 3;
constexpr int SUPPORT_MAX_POINTS = 16;
// rows of the `scalars` output
constexpr int SUPPORT_STABILITY_MARGIN = 0, SUPPORT_REWARD_ROBUSTNESS = 1;

// Validate a description and pack it.  Returns false and a message on a malformed description.
inline bool support_pack(const jm_support_desc * d, std::vector<int32_t> & it, std::vector<double> & dt, std::string & why)
{
    const std::string who = "jm_support_plan_create: ";
    if (!d) { why = who + "null description"; return false; }
    if (!d->point_column) { why = who + "null array in the description"; return false; }
    if (d->n_frames < 1 || d->n_points < 1 || d->n_points > SUPPORT_MAX_POINTS || d->n_points > d->n_frames)
    { why = who + "bad sizes (1 <= n_points <= " + std::to_string(SUPPORT_MAX_POINTS) + ", n_points <= n_frames)"; return false; }
    if (d->reference_frame != FR_LOCAL && d->reference_frame != FR_LOCAL_WORLD_ALIGNED)
    { why = who + "Reference frame must be either LOCAL (0) or LOCAL_WORLD_ALIGNED (1)."; return false; }
    for (int i = 0; i < d->n_points; ++i)
    {
        const int col = d->point_column[i];
        if (col < 0 || col >= d->n_frames)
        { why = who + "point_column[" + std::to_string(i) + "] = " + std::to_string(col) + " out of range [0, " + std::to_string(d->n_frames) + ")"; return false; }
        for (int g = 0; g < i; ++g)
            if (d->point_column[g] == col)
            { why = who + "point_column[" + std::to_string(i) + "] repeats the column of point " + std::to_string(g); return false; }
    }
    it = {d->n_frames, d->n_points, d->reference_frame};
    it.insert(it.end(), d->point_column, d->point_column + d->n_points);
    dt = {0.0};
    return true;
}

// The cutoffs of one launch: finite and not negative (`MaximizeRobustness.__init__`, compositions/locomotion.py:94-97).
inline bool support_cutoffs_check(double cutoff_inner, double cutoff_outer, std::string & why)
{
    if (!std::isfinite(cutoff_inner) || !std::isfinite(cutoff_outer) || cutoff_inner < 0.0 || cutoff_outer < 0.0)
    { why = "jm_block_support_polygon: The inner and outer cutoff thresholds must both be positive (and finite)."; return false; }
    return true;
}

// the inputs and outputs of one launch (device pointers of the kernel's scalar type but the two int32 outputs); every one
// may be null
template<class T> struct SupportIO
{
    const T * pose;            // [7][K][B] of the frame kinematics block (rows 0 and 1 are read)
    const T * odom_pose;       // [3][B] of the locomotion quantities block (LOCAL only)
    const T * zmp;             // [2][B] of the locomotion quantities block, in the plan's reference frame
    const uint8_t * lane_mask; // [B]
    int32_t * n_vertices;      // [B]
    int32_t * vertex_index;    // [16][B]
    T * vertices;              // [2][16][B]
    T * center;                // [2][B]
    T * scalars;               // [2][B]
};

// what a lane needs to read point `i` of the plan: rows x and y of its column, through `translate_position_odom`
// (common/quantities/locomotion.py:904-910) in LOCAL
template<class T> struct SupportPoints
{
    const int32_t * col;
    const T * x_row;           // row 0 of `pose` at this lane
    const T * y_row;           // row 1
    long long B;
    bool local;
    T ref_x, ref_y, cos_yaw, sin_yaw;
    JM_DEV void read(int i, T & x, T & y) const
    {
        const long long o = (long long)col[i] * B;
        x = x_row[o]; y = y_row[o];
        if (local)
        {
            const T rx = x - ref_x, ry = y - ref_y;
            x = frame_product(cos_yaw * rx) + frame_product(sin_yaw * ry);
            y = frame_product(cos_yaw * ry) - frame_product(sin_yaw * rx);
        }
    }
};

// the order of the two stable sorts (math/qhull.py:71-72): a NaN behind every number, as numpy sorts
template<class T> JM_DEV bool support_before(T a, T b) { return a < b || (b != b && a == a); }
// point j (xj, yj) comes before point i: by y, then by x, then by index
template<class T> JM_DEV bool support_key_before(T xj, T yj, int j, T xi, T yi, int i)
{
    if (support_before(yj, yi)) return true;
    if (support_before(yi, yj)) return false;
    if (support_before(xj, xi)) return true;
    if (support_before(xi, xj)) return false;
    return j < i;
}

// a list of at most 16 indices of 4 bits in one register
JM_DEV int support_get(unsigned long long list, int k) { return (int)((list >> (4 * k)) & 0xFull); }
JM_DEV unsigned long long support_put(unsigned long long list, int k, int index) { return list | ((unsigned long long)index << (4 * k)); }
JM_DEV unsigned long long support_keep(unsigned long long list, int len) { return len >= 16 ? list : list & ((1ull << (4 * len)) - 1ull); }

// One monotone chain (math/qhull.py:90-101 downwards through the order, :112-122 upwards).  Returns the stack (its first
// entry is the chain's first point, which is not a vertex of this chain) and its length.  `a` is the entry below the top,
// `b` the top.  The two predicates of the reference differ in the order of the factors of their right-hand side only,
// which a product does not see.
template<class T> JM_DEV unsigned long long support_chain(const SupportPoints<T> & pts, unsigned long long order, int n, bool reversed, int & len)
{
    unsigned long long stack = 0ull;
    len = 0;
    T ax = T(0), ay = T(0), bx = T(0), by = T(0);
    for (int k = 0; k < n; ++k)
    {
        const int i = support_get(order, reversed ? n - 1 - k : k);
        T px, py;
        pts.read(i, px, py);
        // `while len(chain) > 1`: at most len - 1 pops
        for (int t = len; t > 1; --t)
        {
            if ((bx - ax) * (py - ay) > (px - ax) * (by - ay)) break;
            --len;
            stack = support_keep(stack, len);
            bx = ax; by = ay;
            if (len > 1) pts.read(support_get(stack, len - 2), ax, ay);
        }
        stack = support_put(stack, len, i);
        ++len;
        ax = bx; ay = by; bx = px; by = py;
    }
    return stack;
}

// `np.maximum` / `np.minimum` (a NaN wins)
template<class T> JM_DEV T support_clip01(T r)
{
    r = (r > T(0) || r != r) ? r : T(0);
    return (r < T(1) || r != r) ? r : T(1);
}

// All quantities of one lane.  A part whose inputs or output are null is skipped.
template<class T>
JM_DEV void support_lane(const int32_t * __restrict__ it, const SupportIO<T> & io, T cutoff_inner, T cutoff_outer, long long B, long long lane)
{
    if (!io.pose) return;
    const int K = it[0], n = it[1];
    const long long KB = (long long)K * B, MB = (long long)SUPPORT_MAX_POINTS * B;
    SupportPoints<T> pts;
    pts.col = it + SUPPORT_HEAD_INTS;
    pts.x_row = io.pose + lane; pts.y_row = io.pose + KB + lane;
    pts.B = B;
    pts.local = it[2] == FR_LOCAL;
    pts.ref_x = pts.ref_y = pts.sin_yaw = T(0); pts.cos_yaw = T(1);
    if (pts.local)
    {
        if (!io.odom_pose) return;      // (the polygon of the odometry frame needs the odometry pose)
        pts.ref_x = io.odom_pose[lane]; pts.ref_y = io.odom_pose[B + lane];
        sincos_(io.odom_pose[2 * B + lane], &pts.sin_yaw, &pts.cos_yaw);
    }

    // the order (math/qhull.py:71-72): the rank of every point is the number of points before it
    unsigned long long order = 0ull;
    for (int i = 0; i < n; ++i)
    {
        T xi, yi;
        pts.read(i, xi, yi);
        int rank = 0;
        for (int j = 0; j < n; ++j)
        {
            T xj, yj;
            pts.read(j, xj, yj);
            rank += (j != i && support_key_before(xj, yj, j, xi, yi, i)) ? 1 : 0;
        }
        order = support_put(order, rank, i);
    }

    // the vertices (:75-77; :82-123: the upper chain over the reversed order, then the lower chain, each without its first point)
    unsigned long long verts = order;
    int nv = n;
    if (n > 3)
    {
        int len_upper, len_lower;
        const unsigned long long upper = support_chain(pts, order, n, true, len_upper);
        const unsigned long long lower = support_chain(pts, order, n, false, len_lower);
        const int n_upper = len_upper - 1;                      // (in 1 .. 15)
        verts = (upper >> 4) | ((lower >> 4) << (4 * n_upper));
        nv = n_upper + len_lower - 1;
        nv = nv < SUPPORT_MAX_POINTS ? nv : SUPPORT_MAX_POINTS;
    }

    const T nan = T(__builtin_nanf(""));
    if (io.n_vertices) io.n_vertices[lane] = nv;
    // `ConvexHull2D.center` (:396-414): the mean of the vertices
    T sx = T(0), sy = T(0);
    for (int k = 0; k < SUPPORT_MAX_POINTS; ++k)
    {
        const bool on = k < nv;
        const int i = on ? support_get(verts, k) : -1;
        T vx = nan, vy = nan;
        if (on)
        {
            pts.read(i, vx, vy);
            sx = k == 0 ? vx : sx + vx; sy = k == 0 ? vy : sy + vy;
        }
        if (io.vertex_index) io.vertex_index[(long long)k * B + lane] = i;
        if (io.vertices) { io.vertices[(long long)k * B + lane] = vx; io.vertices[MB + (long long)k * B + lane] = vy; }
    }
    if (io.center) { io.center[lane] = sx / T(nv); io.center[B + lane] = sy / T(nv); }

    if (!io.zmp || !io.scalars) return;
    const T qx = io.zmp[lane], qy = io.zmp[B + lane];
    // `ConvexHull2D.get_distance_to_point` (:416-457)
    T distance;
    if (n > 2)
    {
        // `compute_vectors_from_convex` (:143-145): edge k runs from vertex k to vertex k - 1 (edge 0: to the last one);
        // `compute_distance_convex_to_point` (:209-224)
        T prev_x, prev_y;
        pts.read(support_get(verts, nv - 1), prev_x, prev_y);
        bool inside = true;
        T best = T(0);
        for (int k = 0; k < nv; ++k)
        {
            T vx, vy;
            pts.read(support_get(verts, k), vx, vy);
            const T ex = prev_x - vx, ey = prev_y - vy, rx = qx - vx, ry = qy - vy;
            inside = inside && (rx * ey > ry * ex);
            const T ratio = support_clip01((rx * ex + ry * ey) / (ex * ex + ey * ey));
            const T dx = qx - (ratio * ex + vx), dy = qy - (ratio * ey + vy);
            const T d2 = dx * dx + dy * dy;
            // `np.min` (a NaN wins)
            best = (k == 0 || d2 < best || d2 != d2) ? d2 : best;
            prev_x = vx; prev_y = vy;
        }
        distance = (T(1) - T(2) * (inside ? T(1) : T(0))) * sqrt_(best);
    }
    else if (n == 2)
    {
        // the distance to the segment (:444-448)
        T x0, y0, x1, y1;
        pts.read(support_get(verts, 0), x0, y0);
        pts.read(support_get(verts, 1), x1, y1);
        const T ex = x1 - x0, ey = y1 - y0;
        const T ratio = support_clip01(((qx - x0) * ex + (qy - y0) * ey) / (ex * ex + ey * ey));
        const T dx = qx - (x0 + ratio * ex), dy = qy - (y0 + ratio * ey);
        distance = sqrt_(dx * dx + dy * dy);
    }
    else
    {
        // the distance to the point (:451-452)
        T x0, y0;
        pts.read(support_get(verts, 0), x0, y0);
        const T dx = qx - x0, dy = qy - y0;
        distance = sqrt_(dx * dx + dy * dy);
    }
    // `StabilityMarginProjectedSupportPolygon.refresh` (quantities/locomotion.py:228-239)
    const T margin = qx != qx ? -T(__builtin_inff()) : -distance;
    io.scalars[(long long)SUPPORT_STABILITY_MARGIN * B + lane] = margin;
    // `sigmoid_normalization(margin, -cutoff_outer, cutoff_inner, is_asymmetric=True)` (compositions/locomotion.py:39-48)
    if (cutoff_inner > T(0) && cutoff_outer > T(0))
    {
        const T cutoff_low = -cutoff_outer, cutoff_high = cutoff_inner;
        const T value_rel = margin * cutoff_high > T(0) ? margin / cutoff_high : -margin / cutoff_low;
        const T factor = loco_pow(T(LOCO_CUTOFF_ESP) / (T(1) - T(LOCO_CUTOFF_ESP)), fabs_(value_rel));
        io.scalars[(long long)SUPPORT_REWARD_ROBUSTNESS * B + lane] = value_rel > T(0) ? T(1) / (T(1) + factor) : factor / (T(1) + factor);
    }
}

#ifndef JM_HOST_EMU
template<class T>
__global__ void __launch_bounds__(256) k_support_polygon(const int32_t * __restrict__ it, const SupportIO<T> io, double cutoff_inner,
                                                          double cutoff_outer, long long B)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= B) return;
    if (io.lane_mask && !io.lane_mask[lane]) return;
    support_lane<T>(it, io, (T)cutoff_inner, (T)cutoff_outer, B, lane);
}
#endif
}  // namespace jm
