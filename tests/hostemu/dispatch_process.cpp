// dispatch_process.cpp -- jm_dispatch.h with the `process` fact (process forces registered) behind a C interface for
// tests/test_process_forces.py.  Host only: the header includes nothing of HIP.
#include "../../jiminy_amd/csrc/jm_dispatch.h"

namespace jd = jm::dispatch;

extern "C" int dispatch_process_select(const int * t, int mode, int family, long long B, int f64, int constraint, int applied,
                                       int process, const char ** refusal)
{
    const jd::Traits traits = {t[0] != 0, t[1] != 0, t[2] != 0, t[3], t[4] != 0};
    // a default-configured process: float64 or not, every split switch on, nothing else bound
    jd::Facts f = {};
    f.mode = mode; f.family = family; f.n_cus = 256; f.B = B;
    f.f64 = f64 != 0; f.constraint = constraint != 0; f.con_rows = true;
    f.applied = applied != 0; f.process = process != 0;
    f.split = true; f.split_start = true;
    const jd::Selection s = jd::select_form(traits, f);
    *refusal = s.refusal;
    return (int)s.form;
}
