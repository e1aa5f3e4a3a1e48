// jm_ground.h -- the ground under a point: the height map of `set_ground_heightmap` as bilinear patches (height and unit
// normal, flat continuation outside the map) and the tangents of the local frame of a contact constraint on that surface.
// One definition for the physics kernels (jm_kernels.h, jm_constraint.h, jm_quad.h) and the locomotion quantities
// (jm_locomotion.h).
#pragma once
#include "jm_math.h"

namespace jm
{
// world.groundProfile(x, y) -> height and unit normal out of the height map of the batch arguments
// (`A`: anything with the height-map fields of BatchArgs -- the batch arguments or the constraint arguments)
template<class T, class G> JM_DEV void ground_profile(const G & A, T x, T y, T & h, V3<T> & n)
{
    const int nx = A.ground_nx, ny = A.ground_ny;
    T u = (x - A.ground_x0) / A.ground_dx, w = (y - A.ground_y0) / A.ground_dy;
    const bool in_x = u >= T(0) && u <= T(nx - 1), in_y = w >= T(0) && w <= T(ny - 1);
    u = fmin_(fmax_(u, T(0)), T(nx - 1));
    w = fmin_(fmax_(w, T(0)), T(ny - 1));
    int ix = (int)u, iy = (int)w;
    ix = ix > nx - 2 ? nx - 2 : ix; iy = iy > ny - 2 ? ny - 2 : iy;
    ix = ix < 0 ? 0 : ix; iy = iy < 0 ? 0 : iy;
    const T fx = u - T(ix), fy = w - T(iy);
    const T h00 = A.ground_h[iy * nx + ix], h10 = A.ground_h[iy * nx + ix + 1];
    const T h01 = A.ground_h[(iy + 1) * nx + ix], h11 = A.ground_h[(iy + 1) * nx + ix + 1];
    h = (T(1) - fy) * ((T(1) - fx) * h00 + fx * h10) + fy * ((T(1) - fx) * h01 + fx * h11);
    // outside the grid the ground continues flat (height of the nearest edge sample, no slope across the edge)
    const T dhdx = in_x ? ((T(1) - fy) * (h10 - h00) + fy * (h11 - h01)) / A.ground_dx : T(0);
    const T dhdy = in_y ? ((T(1) - fx) * (h01 - h00) + fx * (h11 - h10)) / A.ground_dy : T(0);
    const T inv = T(1) / sqrt_(dhdx * dhdx + dhdy * dhdy + T(1));
    n = {-dhdx * inv, -dhdy * inv, inv};
}

// The tangents of `rotationLocal_` = [t0 t1 n] of a contact constraint on a surface of unit normal n
// (FrameConstraint::setNormal, frame_constraint.cc:62-68): t1 = normalize(n x e_x) = (0, n.z, -n.y) / |.|, t0 = t1 x n
template<class T> JM_DEV void ground_tangents(V3<T> n, V3<T> & t0, V3<T> & t1)
{
    const T inv = rsqrt_(n.z * n.z + n.y * n.y);
    t1 = {T(0), n.z * inv, -n.y * inv};
    t0 = cross(t1, n);
}
}  // namespace jm
