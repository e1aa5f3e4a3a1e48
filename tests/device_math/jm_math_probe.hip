// Probe of the device math layer (tests only): every primitive of jiminy_amd/csrc/jm_math.h applied lane by lane to
// arrays, in float64 and float32.  Compiled twice from this one text:
//   * for gfx950 with the kernels' own flags (jiminy_amd/codegen.py build_probe): the launchers take device pointers;
//   * by the host emulation's compiler and flags with -DJM_HOST_EMU (tests/device_math/probe.py): the same launchers
//     loop over host arrays.
// Row i of `in` holds the NIN[op] inputs of lane i, row i of `out` its NOUT[op] outputs.  Modes:
//   0  every lane active (blocks of 256);
//   1  divergent: lanes with i % 3 == 1 skip the call and leave their output row untouched;
//   2  ragged: blocks of 64 and a length that is not a multiple of 64 (the tail of the last wavefront idles).
// Consumer: tests/test_device_math.py.
#include "../../jiminy_amd/csrc/jm_math.h"

#ifdef JM_HOST_EMU
#define PROBE_KERNEL static
#else
#define PROBE_KERNEL __global__
#endif

namespace
{
using namespace jm;

enum Op { SINCOS, TANH, RCP, RSQRT, SQRT, EXP6, LOG3, MATRIX_TO_QUAT, QUAT_TO_MATRIX, QUAT_EXP3, QUAT_LOG3, QUAT_MUL,
          JLOG3_MUL, SYM_INVERSE, ROT_RODRIGUES, N_OPS };
constexpr int NIN[N_OPS] = {1, 1, 1, 1, 1, 6, 9, 9, 4, 3, 4, 8, 7, 6, 5};
constexpr int NOUT[N_OPS] = {2, 1, 1, 1, 1, 12, 3, 4, 9, 4, 4, 4, 3, 6, 9};

template<class T> JM_DEV M3<T> m3_of(const T * a) { return {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]}; }
template<class T> JM_DEV void put_m3(const M3<T> & R, T * o)
{
    o[0] = R.m00; o[1] = R.m01; o[2] = R.m02; o[3] = R.m10; o[4] = R.m11; o[5] = R.m12; o[6] = R.m20; o[7] = R.m21; o[8] = R.m22;
}
template<class T> JM_DEV void put_v3(V3<T> v, T * o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

template<class T, int OP> JM_DEV void apply(const T * a, T * o)
{
    if constexpr (OP == SINCOS) sincos_(a[0], &o[0], &o[1]);
    else if constexpr (OP == TANH) o[0] = tanh_(a[0]);
    else if constexpr (OP == RCP) o[0] = rcp_(a[0]);
    else if constexpr (OP == RSQRT) o[0] = rsqrt_(a[0]);
    else if constexpr (OP == SQRT) o[0] = sqrt_(a[0]);
    else if constexpr (OP == EXP6)
    {
        const SE3<T> M = exp6(Sp<T>{V3<T>{a[0], a[1], a[2]}, V3<T>{a[3], a[4], a[5]}});
        put_m3(M.R, o);
        put_v3(M.p, o + 9);
    }
    else if constexpr (OP == LOG3) put_v3(log3(m3_of(a)), o);
    else if constexpr (OP == MATRIX_TO_QUAT) matrix_to_quat(m3_of(a), o[0], o[1], o[2], o[3]);
    else if constexpr (OP == QUAT_TO_MATRIX) put_m3(quat_to_matrix(a[0], a[1], a[2], a[3]), o);
    else if constexpr (OP == QUAT_EXP3)
    {
        T q[4];
        quat_exp3(V3<T>{a[0], a[1], a[2]}, q);
        for (int k = 0; k < 4; ++k) o[k] = q[k];
    }
    else if constexpr (OP == QUAT_LOG3)
    {
        T theta;
        put_v3(quat_log3(a[0], a[1], a[2], a[3], theta), o);
        o[3] = theta;
    }
    else if constexpr (OP == QUAT_MUL)
    {
        const T b[4] = {a[4], a[5], a[6], a[7]};
        T r[4];
        quat_mul(a, b, r);
        for (int k = 0; k < 4; ++k) o[k] = r[k];
    }
    else if constexpr (OP == JLOG3_MUL) put_v3(jlog3_mul(a[0], V3<T>{a[1], a[2], a[3]}, V3<T>{a[4], a[5], a[6]}), o);
    else if constexpr (OP == SYM_INVERSE)
    {
        const S3<T> S = sym_inverse(S3<T>{a[0], a[1], a[2], a[3], a[4], a[5]});
        o[0] = S.xx; o[1] = S.xy; o[2] = S.xz; o[3] = S.yy; o[4] = S.yz; o[5] = S.zz;
    }
    else if constexpr (OP == ROT_RODRIGUES) put_m3(rot_rodrigues(V3<T>{a[0], a[1], a[2]}, a[3], a[4]), o);
}

// one lane: the call sits inside the divergent branch, like the contact law's, and so do the stores of its outputs
template<class T, int OP> JM_DEV void lane(const T * in, T * out, int i, int mode)
{
    if (mode != 1 || i % 3 != 1)
    {
        T o[NOUT[OP]];
        apply<T, OP>(in + (long long)i * NIN[OP], o);
        for (int k = 0; k < NOUT[OP]; ++k) out[(long long)i * NOUT[OP] + k] = o[k];
    }
}

#ifdef JM_HOST_EMU
template<class T, int OP> int launch(const T * in, T * out, int n, int mode)
{
    for (int i = 0; i < n; ++i) lane<T, OP>(in, out, i, mode);
    return 0;
}
#else
template<class T, int OP> __global__ void k_probe(const T * in, T * out, int n, int mode)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lane<T, OP>(in, out, i, mode);
}
template<class T, int OP> int launch(const T * in, T * out, int n, int mode)
{
    const int block = mode == 2 ? 64 : 256;
    k_probe<T, OP><<<(n + block - 1) / block, block>>>(in, out, n, mode);
    const hipError_t e = hipDeviceSynchronize();
    return e == hipSuccess ? (int)hipGetLastError() : (int)e;
}
#endif

template<class T> int dispatch(int op, const T * in, T * out, int n, int mode)
{
    if (n < 0 || mode < 0 || mode > 2 || (mode == 2 && n % 64 == 0)) return -1;
    if (n == 0) return 0;
    switch (op)
    {
    case SINCOS: return launch<T, SINCOS>(in, out, n, mode);
    case TANH: return launch<T, TANH>(in, out, n, mode);
    case RCP: return launch<T, RCP>(in, out, n, mode);
    case RSQRT: return launch<T, RSQRT>(in, out, n, mode);
    case SQRT: return launch<T, SQRT>(in, out, n, mode);
    case EXP6: return launch<T, EXP6>(in, out, n, mode);
    case LOG3: return launch<T, LOG3>(in, out, n, mode);
    case MATRIX_TO_QUAT: return launch<T, MATRIX_TO_QUAT>(in, out, n, mode);
    case QUAT_TO_MATRIX: return launch<T, QUAT_TO_MATRIX>(in, out, n, mode);
    case QUAT_EXP3: return launch<T, QUAT_EXP3>(in, out, n, mode);
    case QUAT_LOG3: return launch<T, QUAT_LOG3>(in, out, n, mode);
    case QUAT_MUL: return launch<T, QUAT_MUL>(in, out, n, mode);
    case JLOG3_MUL: return launch<T, JLOG3_MUL>(in, out, n, mode);
    case SYM_INVERSE: return launch<T, SYM_INVERSE>(in, out, n, mode);
    case ROT_RODRIGUES: return launch<T, ROT_RODRIGUES>(in, out, n, mode);
    default: return -1;
    }
}
}  // namespace

// (op, inputs, outputs, lanes, mode) -> 0 on success; pointers are device pointers in the gfx950 build
extern "C" int jm_probe_f64(int op, const double * in, double * out, int n, int mode) { return dispatch<double>(op, in, out, n, mode); }
extern "C" int jm_probe_f32(int op, const float * in, float * out, int n, int mode) { return dispatch<float>(op, in, out, n, mode); }
extern "C" int jm_probe_arity(int op, int which) { return op < 0 || op >= N_OPS ? -1 : (which ? NOUT[op] : NIN[op]); }
