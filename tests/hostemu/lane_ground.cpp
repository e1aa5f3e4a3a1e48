// Host emulation of the one-robot-per-lane constraint kernel on a height-map ground (tests only): the code of emu.cpp
// plus an entry that runs the variation instantiation (`lane_run<..., WithConA>`, what the library launches as
// `k_constrained<double, Topo, true>`) with the map -- and the per-lane patch offsets -- in the batch arguments.
// Options, constraint state and the map come through emu.cpp's setters (emu_set_constraints, emu_set_gen,
// emu_set_ground_offset, emu_set_friction, emu_set_flexibility).
#include "emu.cpp"

extern "C" int emu_run_lane_ground(const jm_model_desc * d, const jm_options * o, const emu_io * io, int mode, int solver,
                                   double dt, int n_sub, int command_changed, int update_sensors)
{
    using T = double;
    if constexpr (Topo::QUAD) return JM_ENOTIMPL;   // (the branch-parallel topologies have kernels of their own)
    if (g_copt.contact_model != JM_CONTACT_CONSTRAINT || !g_con_flags || !g_con_data) return JM_ECONTROLFLOW;
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
    A.flex_lane = (const T *)g_flex_lane;
    A.model_lane = (const T *)g_model_lane;
    A.ground_h = (const T *)g_ground; A.ground_nx = g_gnx; A.ground_ny = g_gny;
    A.ground_off = g_ground ? (const T *)g_ground_off : nullptr;
    A.ground_x0 = (T)g_gx0; A.ground_y0 = (T)g_gy0; A.ground_dx = (T)g_gdx; A.ground_dy = (T)g_gdy;
    A.applied = (const T *)g_applied; A.applied_k = g_applied_k;
    for (int i = 0; i < 12; ++i) A.applied_p[i] = (T)g_applied_p[i];
    for (int i = 0; i < 4; ++i) A.applied_joint[i] = g_applied_joint[i];
    std::vector<T> sb(jm::lane_rows<T, Topo>() + 1, (T)std::nan(""));
    std::vector<T> wsp((size_t)(jm::ConRows<Topo>::WTOTAL + 1) * io->B, (T)std::nan(""));
    jm::ConArgs<T> C;
    C.flags = (int32_t *)g_con_flags; C.data = (T *)g_con_data; C.ws = wsp.data();
    C.friction = (const T *)g_friction;
    const double omega = 2.0 * 3.14159265358979323846 * g_copt.stabilization_freq;
    C.kp = (T)(omega * omega); C.kd = (T)(2.0 * omega);
    const double omega_u = 2.0 * 3.14159265358979323846 * g_copt.user_stabilization_freq;
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
    return 0;
}
