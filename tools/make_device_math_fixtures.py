"""High-precision expected values of the device math layer (jiminy_amd/csrc/jm_math.h) -> tests/golden/device_math.npz.

For every primitive and precision the fixture holds the inputs (the edges where such functions break: reduction
boundaries, Taylor thresholds and their neighbouring floats, special values), the value mpmath computes at 60 digits
as a double-double (`_hi`, `_lo`), and for the composites the float64 value of the reference's formula (`_ref`,
tests/device_math/reference.py).  The doubles next to k pi/2 (every k with k pi/2 < 1e5) are stored compactly: their
offset in ulps from the double nearest to k * (pi/2 rounded); their truth follows exactly from k and x
(reference.kgrid_truth).

    python tools/make_device_math_fixtures.py           # write the fixture
    python tools/make_device_math_fixtures.py --check   # regenerate and compare bit for bit, write nothing
Consumer: tests/test_device_math.py.
"""
from __future__ import annotations

import io
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "device_math.npz")

from tests.device_math import reference as R  # noqa: E402

DTYPES = {"f64": np.float64, "f32": np.float32}


def _near(x, n, dtype):
    """x and its n neighbouring floats of `dtype` on each side."""
    x = np.asarray(x, dtype=dtype)
    out = [x]
    up, dn = x.copy(), x.copy()
    for _ in range(n):
        up, dn = np.nextafter(up, dtype(np.inf)), np.nextafter(dn, dtype(-np.inf))
        out += [up, dn]
    return np.concatenate([o.ravel() for o in out])


def _specials(dtype):
    tiny = np.finfo(dtype).smallest_subnormal
    return np.array([0.0, -0.0, tiny, -tiny, 4 * tiny, np.finfo(dtype).tiny, np.inf, -np.inf, np.nan], dtype=dtype)


def _to_dd(mp, v):
    """mpf -> (hi, lo) float64, both rounded to nearest; non-finite values pass through in hi."""
    from mpmath import libmp
    if not mp.isfinite(v):
        return float(v), 0.0
    hi = libmp.to_float(v._mpf_, rnd="n")
    return hi, libmp.to_float((v - mp.mpf(hi))._mpf_, rnd="n")


def scalar_inputs(rng, dtype):
    ln2 = math.log(2.0)
    big = 1e5 if dtype == np.float64 else 1e4
    logs = _geom(1e-300 if dtype == np.float64 else 1e-37, big, 1200)
    sgn = np.where(rng.random(logs.size) < 0.5, -1.0, 1.0)
    k = np.arange(1, 6367, 7)   # (float32: doubles of k pi/2 rounded to float and their neighbours; float64 has its own grid)
    sincos = np.concatenate([_near([big, -big], 3, dtype), _specials(dtype), logs * sgn, rng.uniform(-big, big, 600),
                             [] if dtype == np.float64 else _near(k * (np.pi / 2), 1, dtype)])
    n = np.arange(0, 59)
    bounds = (n + 0.5) * ln2 / 2
    tanh = np.concatenate([_near(bounds, 3, dtype), -bounds, _near([20.0, 19.999, 10.0], 2, dtype), _specials(dtype),
                           _geom(1e-300 if dtype == np.float64 else 1e-37, 30, 800), rng.uniform(0.05, 0.6, 1500), rng.uniform(0.2, 0.3, 3000),
                           rng.uniform(0.6, 20, 500)])
    lim = 500 if dtype == np.float64 else 100
    e = np.arange(-lim, lim + 1, dtype=np.float64)
    eps = np.finfo(dtype).eps
    mant = np.concatenate([np.ones_like(e), np.full_like(e, 1 + eps), np.full_like(e, 2 - eps)])
    recip = np.concatenate([mant * np.tile(2.0 ** e, 3), np.array([2.0 ** u for u in rng.uniform(-lim, lim, 600)])])
    rspec = np.array([0.0, -0.0, np.inf, np.finfo(dtype).smallest_subnormal, 4 * np.finfo(dtype).smallest_subnormal,
                      np.finfo(dtype).tiny, np.finfo(dtype).max], dtype=np.float64)
    return {"sincos": sincos, "tanh": tanh, "rcp": np.concatenate([recip, -recip[:50], rspec, [-np.inf, np.nan]]),
            "rsqrt": np.concatenate([recip, rspec, [np.nan]]), "sqrt": np.concatenate([recip, rspec, [-1.0, np.nan]])}


def scalar_truth(mp, op, x):
    xm = mp.mpf(float(x))
    if op == "sincos":
        return [mp.sin(xm), mp.cos(xm)]
    if op == "tanh":
        return [mp.tanh(xm)]
    if op == "sqrt":
        return [mp.sqrt(xm) if xm >= 0 else mp.nan]
    if op == "rcp":
        return [1 / xm if xm != 0 else mp.inf]
    return [1 / mp.sqrt(xm) if xm > 0 else (mp.inf if xm == 0 else mp.nan)]


def _geom(a, b, n):
    """log-spaced values by libm alone (numpy's vectorised transcendentals may round differently between machines)"""
    return np.array([a * (b / a) ** (i / (n - 1)) for i in range(n)])


def _norm(a):
    return math.sqrt(sum(float(x) * float(x) for x in a))


def _rot(rng, theta, axis=None):
    a = rng.normal(size=3) if axis is None else np.asarray(axis, dtype=np.float64)
    return a / _norm(a) * theta


def _exp_rot(mp, w):
    """exp(w^) at high precision, rounded to doubles (row major)."""
    out, _ = R.exp6(mp, [0, 0, 0] + list(w), np.float64, False)
    return [float(v) for v in out[:9]]


def composite_inputs(mp, rng, dtype):
    thr = R.TAYLOR[dtype]
    f = dtype
    angles = [0.0, 1e-9, 1e-6, thr * 0.5, thr * 0.99, thr, float(np.nextafter(f(thr), f(0))), float(np.nextafter(f(thr), f(1))),
              thr * 1.001, thr * 1.01, thr * 1.2, thr * 1.5, thr * 1.9, 1e-3, 0.1, 1.0, np.pi / 2, np.pi, 2 * np.pi, 50.0]
    exp6, jl, qe = [], [], []
    for th in angles:
        for axis in ([1, 0, 0], [0, 0, 1], None, None):
            w = _rot(rng, th, axis)
            exp6.append(list(rng.normal(size=3) * rng.choice([0.1, 1.0, 10.0])) + list(w))
            jl.append([th] + list(w) + list(rng.normal(size=3)))
    for t2 in [0.0, 1e-12, thr * 0.5, thr, float(np.nextafter(f(thr), f(0))), float(np.nextafter(f(thr), f(1))), thr * 1.001,
               thr * 1.01, thr * 2, 0.1, 1.0, 9.0, np.pi ** 2, 2500.0]:
        for axis in ([0, 1, 0], None, None):
            qe.append(list(_rot(rng, math.sqrt(t2), axis)))
    # log3: Taylor branch, tr >= 3 from rounding, theta at pi - 1e-2 and its neighbours, theta = pi about axes
    l3 = []
    edge = np.pi - 1e-2
    for th in [0.0, 1e-10, 1e-8, 1e-5, thr * 0.9, thr * 1.1, 1e-3, 0.5, 2.0, 3.0, edge, *np.nextafter(edge, [0, 4]),
               edge - 4e-16, edge + 4e-16, edge - 1e-9, edge + 1e-9, np.pi - 1e-4, np.pi - 1e-8, np.pi]:
        for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], None, None):
            l3.append(_exp_rot(mp, _rot(rng, th, axis)))
    # matrix -> quaternion: the four branches, ties (trace = 0, equal diagonals), half turns
    mq = []
    for th, axis in [(0.3, None), (1.0, None), (2 * np.pi / 3, None), (2 * np.pi / 3, [1, 1, 1]), (np.pi, [1, 1, 1]),
                     (np.pi, [1, 0, 0]), (np.pi, [0, 1, 0]), (np.pi, [0, 0, 1]), (np.pi, [1, 1, 0]), (np.pi, [0, 1, 1]),
                     (2.5, [1, 0.1, 0.2]), (2.5, [0.1, 1, 0.2]), (2.5, [0.1, 0.2, 1]), (3.0, None), (3.0, None), (2.9, None)]:
        for _ in range(3):
            mq.append(_exp_rot(mp, _rot(rng, th, axis)))
    q2m, ql, qm = [], [], []
    for _ in range(40):
        q = rng.normal(size=4)
        q2m.append(list(q / _norm(q)))
        qm.append(list(q / _norm(q)) + list(rng.normal(size=4) / 2))
    q2m += [[0, 0, 0, 1], [1, 0, 0, 0], [0.5, 0.5, 0.5, -0.5], list(rng.normal(size=4))]
    for n2 in [0.0, 1e-12, thr * 0.5, thr, float(np.nextafter(f(thr), f(0))), float(np.nextafter(f(thr), f(1))), thr * 1.001,
               thr * 1.01, 0.1, 0.5, 0.99, 1.0]:
        for sw in (1.0, -1.0):
            v = _rot(rng, math.sqrt(n2))
            ql.append(list(v) + [sw * np.sqrt(max(1.0 - n2, 0.0))])
    si, rr = [], []
    for cond in [1.0, 10.0, 1e3, 1e6, 1e8, 1e10]:
        for _ in range(4):
            Q = _exp_rot(mp, _rot(rng, rng.uniform(0.1, 3.0)))
            sc = rng.choice([1e-3, 1.0, 50.0])
            lam = [sc * s for s in (1.0, cond ** rng.uniform(0, 1), cond)]
            A = [[sum(Q[3 * i + m] * lam[m] * Q[3 * j + m] for m in range(3)) for j in range(3)] for i in range(3)]
            si.append([A[0][0], A[0][1], A[0][2], A[1][1], A[1][2], A[2][2]])
    for th in [0.0, 1e-8, 0.3, 1.0, np.pi / 2, 3.0, np.pi]:
        for _ in range(3):
            a = _rot(rng, 1.0)
            rr.append(list(a) + [math.cos(th), math.sin(th)])
    out = {"exp6": exp6, "log3": l3, "matrix_to_quat": mq, "quat_to_matrix": q2m, "quat_exp3": qe, "quat_log3": ql,
           "quat_mul": qm, "jlog3_mul": jl, "sym_inverse": si, "rot_rodrigues": rr}
    return {k: np.asarray(v, dtype=np.float64).astype(dtype) for k, v in out.items()}


def generate() -> dict:
    mp = R.mp_system(60)
    import mpmath
    arrays = {}
    # doubles next to k pi/2: offsets from the double nearest to k * (pi/2 rounded)
    kmax = int(1e5 / (np.pi / 2))
    k = np.arange(1, kmax + 1)
    base = k * (np.pi / 2)
    lo = np.empty_like(base)
    for i, kk in enumerate(k):
        t = kk * mpmath.pi / 2
        n = mpmath.libmp.to_float(t._mpf_, rnd="n")
        lo[i] = n if mpmath.mpf(n) < t else np.nextafter(n, -np.inf)
    off = lo.view(np.int64) - base.view(np.int64)
    assert np.abs(off).max() < 127
    arrays["sincos_kgrid_n"] = np.array(kmax)
    arrays["sincos_kgrid_off"] = off.astype(np.int8)
    for tag, dtype in DTYPES.items():
        rng = np.random.default_rng(20261016 + (dtype == np.float32))
        for op, x in scalar_inputs(rng, dtype).items():
            x = x.astype(dtype)
            tr = [[_to_dd(mpmath, v) for v in scalar_truth(mpmath, op, xi)] for xi in x]
            if op in ("sincos", "tanh", "sqrt"):      # (mpmath has no signed zero: sin, tanh and sqrt of -0 are -0)
                tr = [[(float(xi), 0.0)] + r[1:] if xi == 0 else r for xi, r in zip(x, tr)]
            arrays[f"{op}_{tag}_x"] = x.reshape(-1, 1)
            arrays[f"{op}_{tag}_hi"] = np.array([[h for h, _ in r] for r in tr])
            arrays[f"{op}_{tag}_lo"] = np.array([[l for _, l in r] for r in tr])
        for op, x in composite_inputs(mp, rng, dtype).items():
            fn = R.COMPOSITES[op]
            ref, hi, lo = [], [], []
            for row in x:
                r, br = fn(R.REF, [float(v) for v in row], dtype)
                t, _ = fn(mp, [float(v) for v in row], dtype, br)
                ref.append(r)
                dd = [_to_dd(mpmath, mpmath.mpf(v) if not isinstance(v, mpmath.mpf) else v) for v in t]
                hi.append([h for h, _ in dd])
                lo.append([l for _, l in dd])
            arrays[f"{op}_{tag}_x"] = x
            arrays[f"{op}_{tag}_hi"] = np.array(hi)
            arrays[f"{op}_{tag}_lo"] = np.array(lo)
            arrays[f"{op}_{tag}_ref"] = np.array(ref, dtype=np.float64)
    return arrays


def _bytes(arrays) -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def main():
    arrays = generate()
    if "--check" in sys.argv:
        with np.load(OUT) as old:
            bad = sorted(set(old.files) ^ set(arrays)) + [k for k in arrays if k in old.files and
                                                          old[k].tobytes() != arrays[k].tobytes()]
        if bad:
            print("device_math.npz differs from a fresh generation:", bad)
            sys.exit(1)
        print(f"device_math.npz: {len(arrays)} arrays regenerated bit for bit")
        return
    data = _bytes(arrays)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {os.path.relpath(OUT, ROOT)}: {len(arrays)} arrays, {len(data)} bytes")


if __name__ == "__main__":
    main()
