// dispatch_dopri_process.cpp -- `select_adaptive_form` of jm_dispatch.h with the `process` fact (process forces registered)
// behind a C interface for tests/test_process_forces_adaptive.py.  Host only: the header includes nothing of HIP.
#include "../../jiminy_amd/csrc/jm_dispatch.h"

namespace jd = jm::dispatch;

extern "C" int dispatch_dopri_process(const int * t, int family, int f64, int constraint, int process, int per_stage)
{
    const jd::Traits traits = {t[0] != 0, t[1] != 0, t[2] != 0, t[3], t[4] != 0};
    // a default-configured process: every split switch on, nothing else bound
    jd::Facts f = {};
    f.mode = 2; f.family = family; f.n_cus = 256; f.B = 65536;
    f.f64 = f64 != 0; f.constraint = constraint != 0; f.con_rows = true;
    f.process = process != 0;
    f.split = true; f.split_start = true;
    return (int)jd::select_adaptive_form(traits, f, per_stage != 0);
}
