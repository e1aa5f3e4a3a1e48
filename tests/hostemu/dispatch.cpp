// dispatch.cpp -- jm_dispatch.h (the launch policy of the C ABI library) behind a C interface for tests/test_dispatch_policy.py.
// Host only: the header includes nothing of HIP.
#include "../../jiminy_amd/csrc/jm_dispatch.h"

namespace jd = jm::dispatch;

namespace
{
jd::Traits traits_of(const int * t) { return {t[0] != 0, t[1] != 0, t[2] != 0, t[3], t[4] != 0}; }
// the members of jd::Facts in the order of their declaration
jd::Facts facts_of(const long long * v)
{
    jd::Facts f = {};
    f.mode = (int)v[0]; f.family = (int)v[1]; f.n_cus = (int)v[2]; f.B = v[3];
    f.f64 = v[4]; f.constraint = v[5]; f.con_rows = v[6];
    f.model_lane = v[7]; f.ground = v[8]; f.applied = v[9]; f.friction = v[10];
    f.joint_locks = v[11]; f.compact = v[12]; f.capturing = v[13]; f.torsion = v[14];
    f.split = v[15]; f.split_start = v[16]; f.split_capture = v[17]; f.cooling = v[18];
    return f;
}
}  // namespace

extern "C"
{
int dispatch_select(const int * traits, const long long * facts, int * counters, const char ** refusal)
{
    const jd::Selection s = jd::select_form(traits_of(traits), facts_of(facts));
    *counters = s.counters;
    *refusal = s.refusal;
    return (int)s.form;
}
int dispatch_adaptive(const int * traits, const long long * facts, int per_stage)
{
    return (int)jd::select_adaptive_form(traits_of(traits), facts_of(facts), per_stage != 0);
}
int dispatch_needs_variation(const int * traits, const long long * facts) { return jd::needs_variation(traits_of(traits), facts_of(facts)); }
int dispatch_lane_history(const int * traits) { return traits_of(traits).lane_history(); }

void * history_new() { return new jd::SplitHistory(); }
void history_free(void * h) { delete (jd::SplitHistory *)h; }
void history_reset(void * h) { ((jd::SplitHistory *)h)->reset(); }
int history_due(void * h) { return ((jd::SplitHistory *)h)->due(); }
void history_absorb(void * h, int slot, const int32_t * st) { ((jd::SplitHistory *)h)->absorb(slot, st); }
int history_allowed(void * h) { return ((jd::SplitHistory *)h)->allowed(); }
int history_take_step(void * h) { return ((jd::SplitHistory *)h)->take_step(); }
int history_slot(void * h) { return ((jd::SplitHistory *)h)->slot(); }
void history_recorded(void * h, int slot) { ((jd::SplitHistory *)h)->recorded(slot); }
// slots that wait for the counters of a step
int history_outstanding(void * h)
{
    int n = 0;
    for (long long s : ((jd::SplitHistory *)h)->step_of) n += s >= 0;
    return n;
}
}
