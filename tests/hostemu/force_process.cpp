// Host emulation of the process forces (tests only): the code of emu.cpp plus
//   emu_process_value   the spline of jm_kernels.h (process_force_value) for one lane and one time, and
//   emu_run_process     one launch of the variation instantiations with process forces in the batch arguments -- the
//                       one-robot-per-lane code (`lane_run<..., NoConA>` / `WithConA`, what the library launches as
//                       `k_batch<double, Topo, true>` / `k_constrained<double, Topo, true>`) or the branch-parallel one
//                       (`k_quad_gen` / `k_quad_con_gen`), float64.
// Options and constraint state come through emu.cpp's setters (emu_set_constraints, ...); the frames and held wrenches are arguments.
#include "emu.cpp"

struct emu_process
{
    int row, n_knots;
    double knot_spacing, scale;
    const double * values;
    const double * grads;
};

// the block of the parameter vector the kernels read the process forces from (jm::ProcBlock): appended to `P`
static int append_process_block(std::vector<double> & P, double * lane_time, int k, const emu_process * p)
{
    auto bits = [](const void * q) { double x; std::memcpy(&x, &q, sizeof(x)); return x; };
    const int off = (int)P.size();
    P.resize(P.size() + jm::JM_PROC_BLOCK, 0.0);
    P[off] = (double)k;
    P[off + 1] = bits(lane_time);
    for (int i = 0; i < k; ++i)
    {
        double * c = P.data() + off + 2 + 6 * i;
        c[0] = (double)p[i].row; c[1] = (double)p[i].n_knots; c[2] = p[i].knot_spacing; c[3] = p[i].scale;
        c[4] = bits(p[i].values); c[5] = bits(p[i].grads);
    }
    return off;
}

extern "C" double emu_process_value(const emu_process * p, long long B, long long lane, double t)
{
    std::vector<double> P(1, 0.0);
    append_process_block(P, nullptr, 1, p);
    return jm::process_force_value<double>(jm::ProcBlock<double>{P.data() + 1}, 0, t, B, lane);
}

extern "C" int emu_run_process(const jm_model_desc * d, const jm_options * o, const emu_io * io, int variant, int mode, int solver,
                               double dt, int n_sub, int command_changed, int update_sensors, double * lane_time, int k,
                               const emu_process * procs, const void * held, int n_frames, const double * offsets, const int * joints)
{
    using T = double;
    if (k < 0 || k > 4 || !lane_time) return JM_EINVAL;
    if (variant == 1 && !Topo::QUAD) return JM_ENOTIMPL;
    std::string why;
    if (!jm::check_topology<Topo>(*d, why)) return JM_ETOPOLOGY;
    std::vector<double> P = jm::pack_model<Topo>(*d);
    jm::pack_options<Topo>(P, *o);
    jm::pack_quad<Topo>(P, *d);
    jm::BatchArgs<T> A;
    std::memset(&A, 0, sizeof(A));
    A.P = P.data();
    A.q = (T *)io->q; A.v = (T *)io->v; A.a = (T *)io->a; A.command = (const T *)io->command;
    A.u_motor = (T *)io->u_motor; A.u = (T *)io->u; A.f_external = (T *)io->f_external;
    A.contact_forces = (T *)io->contact_forces; A.imu = (T *)io->imu; A.force = (T *)io->force;
    A.contact = (T *)io->contact; A.encoder = (T *)io->encoder; A.effort = (T *)io->effort;
    A.energy = (T *)io->energy; A.joint_forces = (T *)io->joint_forces; A.centroidal = (T *)io->centroidal;
    A.status = (int32_t *)io->status;
    A.q_in = (const T *)io->q_in; A.v_in = (const T *)io->v_in; A.a_out = (T *)io->a_out;
    A.mask = (const unsigned char *)io->mask; A.q_init = (const T *)io->q_init; A.v_init = (const T *)io->v_init;
    A.B = io->B; A.mode = mode; A.solver = solver; A.n_sub = n_sub; A.command_changed = command_changed;
    A.update_sensors = update_sensors; A.dt = (T)dt;
    const bool con = g_copt.contact_model == JM_CONTACT_CONSTRAINT;
    if (con && (!g_con_flags || !g_con_data)) return JM_ECONTROLFLOW;
    A.friction = con ? nullptr : (const T *)g_friction;
    A.flex_lane = (const T *)g_flex_lane;
    A.model_lane = (const T *)g_model_lane;
    A.ground_h = (const T *)g_ground; A.ground_nx = g_gnx; A.ground_ny = g_gny;
    A.ground_off = g_ground ? (const T *)g_ground_off : nullptr;
    A.ground_x0 = (T)g_gx0; A.ground_y0 = (T)g_gy0; A.ground_dx = (T)g_gdx; A.ground_dy = (T)g_gdy;
    // the frames of the wrenches; their held values may be absent (null): process forces alone
    if (n_frames < 1 || n_frames > 4) return JM_EINVAL;
    A.applied = (const T *)held; A.applied_k = n_frames;
    for (int i = 0; i < 3 * n_frames; ++i) A.applied_p[i] = (T)offsets[i];
    for (int i = 0; i < 4; ++i) A.applied_joint[i] = i < n_frames ? joints[i] : 1;
    for (int i = 0; i < k; ++i)
        if (procs[i].row < 0 || procs[i].row >= 6 * n_frames) return JM_EINVAL;
    A.proc_off = k > 0 ? append_process_block(P, lane_time, k, procs) : 0;
    A.P = P.data();
    const double omega = 2.0 * 3.14159265358979323846 * g_copt.stabilization_freq;
    const double omega_u = 2.0 * 3.14159265358979323846 * g_copt.user_stabilization_freq;
    if (variant == 1)
    {
        if (con)
        {
            jm::QConArgs<T> C;
            C.flags = (int32_t *)g_con_flags; C.data = (T *)g_con_data; C.ws = nullptr;
            C.friction = (const T *)g_friction;
            C.kp = (T)(omega * omega); C.kd = (T)(2.0 * omega);
            C.kp_lock = g_copt.user_stabilization_freq < 0.0 ? C.kp : (T)(omega_u * omega_u);
            C.kd_lock = g_copt.user_stabilization_freq < 0.0 ? C.kd : (T)(2.0 * omega_u);
            C.torsion = (T)g_copt.torsion; C.reg = (T)g_copt.regularization;
            C.tol_abs = (T)g_copt.tol_abs; C.tol_rel = (T)g_copt.tol_rel; C.iter_max = g_copt.pgs_iter_max;
            C.ground_h = A.ground_h; C.ground_nx = A.ground_nx; C.ground_ny = A.ground_ny;
            C.ground_x0 = A.ground_x0; C.ground_y0 = A.ground_y0; C.ground_dx = A.ground_dx; C.ground_dy = A.ground_dy;
            C.stage = nullptr; C.split_e = 0; C.split_r0 = 0; C.split_r1 = (int)A.B;
            run_quad_con<T, Topo, true>(A, P, C);
        }
        else run_quad<T, Topo, true>(A, P);
        return 0;
    }
    std::vector<T> sb(jm::lane_rows<T, Topo>() + 1, (T)std::nan(""));
    if (con)
    {
        std::vector<T> wsp((size_t)(jm::ConRows<Topo>::WTOTAL + 1) * io->B, (T)std::nan(""));
        jm::ConArgs<T> C;
        C.flags = (int32_t *)g_con_flags; C.data = (T *)g_con_data; C.ws = wsp.data();
        C.friction = (const T *)g_friction;
        C.kp = (T)(omega * omega); C.kd = (T)(2.0 * omega);
        C.kp_lock = g_copt.user_stabilization_freq < 0.0 ? C.kp : (T)(omega_u * omega_u);
        C.kd_lock = g_copt.user_stabilization_freq < 0.0 ? C.kd : (T)(2.0 * omega_u);
        C.torsion = (T)g_copt.torsion; C.reg = (T)g_copt.regularization;
        C.tol_abs = (T)g_copt.tol_abs; C.tol_rel = (T)g_copt.tol_rel; C.iter_max = g_copt.pgs_iter_max;
        std::vector<T> xvec(jm::ConRows<Topo>::NR + 1, (T)std::nan(""));
        C.xl = xvec.data(); C.xstride = 1;
        std::vector<T> yvec(8, (T)std::nan(""));
        C.yl = yvec.data(); C.ystride = 1; C.yrows = 7;
        C.park = nullptr; C.park_rows = 0;
        for (long long lane = 0; lane < io->B; ++lane) jm::lane_run<T, Topo, 1, jm::WithConA>(A, lane, sb.data(), C);
    }
    else
        for (long long lane = 0; lane < io->B; ++lane) jm::lane_run<T, Topo, 1, jm::NoConA>(A, lane, sb.data());
    return 0;
}
