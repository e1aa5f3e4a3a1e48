// Host emulation of the persistent adaptive stepper with process forces (tests only): the code of force_process.cpp plus
//   emu_run_dopri_process   every robot of the batch from its time to `t_next` through `quad_dopri_run<..., GEN = true>` (what
//                           the library launches as `k_quad_dopri_gen`), the process block and the frames of the wrenches in the
//                           batch arguments.  Float64, spring-damper contacts, branch-parallel topologies.
// The per-stage kernels of jm_adaptive.h are device code only and are not part of the emulation.
#include "force_process.cpp"

extern "C" int emu_run_dopri_process(const jm_model_desc * d, const jm_options * o, const emu_io * io, double * fs, int32_t * is,
                                     double t_next, double tol_rel, double tol_abs, double dt_max, double dt_restore,
                                     int succ_failed_max, int new_step, int max_attempts, int32_t * counters, double * lane_time,
                                     int k, const emu_process * procs, const void * held, int n_frames, const double * offsets,
                                     const int * joints)
{
    using T = double;
    if constexpr (Topo::QUAD)
    {
        if (k < 0 || k > 4 || (k > 0 && !lane_time) || n_frames < 1 || n_frames > 4) return JM_EINVAL;
        for (int i = 0; i < k; ++i)
            if (procs[i].row < 0 || procs[i].row >= 6 * n_frames) return JM_EINVAL;
        std::string why;
        if (!jm::check_topology<Topo>(*d, why)) return JM_ETOPOLOGY;
        std::vector<double> P = jm::pack_model<Topo>(*d);
        jm::pack_options<Topo>(P, *o);
        jm::pack_quad<Topo>(P, *d);
        jm::BatchArgs<T> A;
        std::memset(&A, 0, sizeof(A));
        A.q = (T *)io->q; A.v = (T *)io->v; A.a = (T *)io->a; A.command = (const T *)io->command;
        A.status = (int32_t *)io->status;
        A.B = io->B; A.mode = jm::MODE_DYNAMICS;
        A.applied = (const T *)held; A.applied_k = n_frames;
        for (int i = 0; i < 3 * n_frames; ++i) A.applied_p[i] = (T)offsets[i];
        for (int i = 0; i < 4; ++i) A.applied_joint[i] = i < n_frames ? joints[i] : 1;
        A.proc_off = k > 0 ? append_process_block(P, lane_time, k, procs) : 0;
        A.P = P.data();
        std::vector<T> ws((size_t)(jm::AdaptiveRows<Topo>::TOTAL + 1) * io->B, std::nan(""));
        jm::AdaptiveArgs<T> D;
        std::memset(&D, 0, sizeof(D));
        D.P = P.data(); D.q = A.q; D.v = A.v; D.a = A.a; D.ws = ws.data(); D.command = A.command;
        D.fs = fs; D.is = is; D.status = A.status; D.n_active = counters; D.B = io->B;
        D.t_next = t_next; D.tol_rel = tol_rel; D.tol_abs = tol_abs; D.dt_max = dt_max; D.dt_restore_threshold_rel = dt_restore;
        D.succ_failed_max = succ_failed_max; D.new_step = new_step;
        counters[0] = counters[1] = 0;
        QuadShared sh;
        pthread_barrier_init(&sh.bar, nullptr, 4);
        const T * table = P.data() + jm::QLayout<Topo>::OFFSET;
        std::vector<std::thread> th;
        for (int q = 0; q < 4; ++q)
            th.emplace_back([&, q]() {
                HostQuad::sh = &sh;
                HostQuad::k = q;
                std::vector<T> sl(jm::QRows<Topo>::NL + 1, std::nan("")), sb(jm::QDopriRows<Topo>::NB + 1, std::nan(""));
                const jm::StageBuf<T, 1, 1> S{sl.data(), sb.data(), true};
                for (long long r = 0; r < A.B; ++r) jm::quad_dopri_run<T, Topo, HostQuad, 1, 1, true>(A, D, r, q, table, S, max_attempts);
            });
        for (auto & t : th) t.join();
        pthread_barrier_destroy(&sh.bar);
        return 0;
    }
    else
    {
        (void)d; (void)o; (void)io; (void)fs; (void)is; (void)t_next; (void)tol_rel; (void)tol_abs; (void)dt_max; (void)dt_restore;
        (void)succ_failed_max; (void)new_step; (void)max_attempts; (void)counters; (void)lane_time; (void)k; (void)procs; (void)held;
        (void)n_frames; (void)offsets; (void)joints;
        return JM_ENOTIMPL;
    }
}
