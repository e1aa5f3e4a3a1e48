"""The device math layer (jiminy_amd/csrc/jm_math.h) against high-precision values (tests/golden/device_math.npz,
tools/make_device_math_fixtures.py), through the probe tests/device_math/jm_math_probe.hip:

* accuracy contracts of the scalar primitives, in ulps of the correctly rounded value, special values bit for bit;
* faithfulness of the Pinocchio / Eigen composites: within a few ulps of the reference's own float64 formula, and no
  farther from the truth than that formula plus a few ulps (the reference's cancellation is allowed, no more);
* (gpu) the gfx950 build: the same bits whether every lane, a divergent subset or a ragged tail runs the call, and the
  same results as the host twin within the stated bounds -- bit for bit where recorded in BIT_EXACT.

The CPU leg runs the same checks on the host twin (the same source built by the host emulation's compiler).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests.device_math import probe
from tests.device_math import reference as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_math.npz")
TAGS = {"f64": np.float64, "f32": np.float32}
SCALARS = ("sincos", "tanh", "rcp", "rsqrt", "sqrt")

# accuracy contracts (ulps of the output precision), as the comments of jm_math.h state them; float32 bounds are the
# measured maxima of the gfx950 build (its ocml sinf / cosf / tanhf) rounded up
CONTRACT = {("sincos", "f64"): 2.0, ("tanh", "f64"): 3.0, ("rcp", "f64"): 1.0, ("rsqrt", "f64"): 1.0, ("sqrt", "f64"): 0.5,
            ("sincos", "f32"): 2.0, ("tanh", "f32"): 2.0, ("rcp", "f32"): 0.5, ("rsqrt", "f32"): 1.5, ("sqrt", "f32"): 0.5}
# (float32 rsqrt_ is 1.0f / sqrtf(x): two roundings)
# the host twin's rsqrt_ is 1 / sqrt(x): two roundings
HOST_CONTRACT = {("rsqrt", "f64"): 1.5, ("tanh", "f32"): 2.5}   # (and tanhf is glibc's)
# where each contract holds: sincos_ f64 below its cutoff 1e5 (NaN at and beyond it), rcp_ / rsqrt_ f64 on [2^-500, 2^500]
DOMAIN = {"sincos": lambda x, t: np.abs(x) < (1e5 if t == "f64" else np.inf),
          "tanh": lambda x, t: np.isfinite(x),
          "rcp": lambda x, t: (np.abs(x) >= 2.0 ** -500) & (np.abs(x) <= 2.0 ** 500) if t == "f64" else
          np.isfinite(x) & (np.abs(x) >= np.finfo(np.float32).tiny),
          "rsqrt": lambda x, t: (x >= 2.0 ** -500) & (x <= 2.0 ** 500) if t == "f64" else
          np.isfinite(x) & (x >= np.finfo(np.float32).tiny),
          "sqrt": lambda x, t: np.isfinite(x) & (x >= 0)}
# the composites, in ulps of the largest |truth| of an output group: |got - ref64| (f64) and the allowance beyond the
# reference's own distance to the truth (f64), the distance to the truth in float32 ulps (f32, measured maxima rounded up)
FAITH_REF = 4.0
FAITH_TRUTH = 4.0
# (the float32 formulas cancel as the reference's do: log3 / quat_log3 / jlog3_mul near their thresholds and near pi,
# sym_inverse: in units of the cofactor formula's error bound)
FAITH_REF_OP = {"exp6": 16.0, "jlog3_mul": 256.0}    # (t -> 1 - cos t and 1 - sin t / t amplify a 1-ulp difference of sincos_ and libm by ~1/t)
# float32: |got - the reference's formula in float32| in float ulps (exp6: the contracted p = a_v v + ... cancels)
F32_REF = {"exp6": 16.0}
F32_TRUTH = {"exp6": 128.0, "log3": 4096.0, "matrix_to_quat": 4.0, "quat_to_matrix": 4.0, "quat_exp3": 32.0, "quat_log3": 4096.0,
             "quat_mul": 4.0, "jlog3_mul": 4096.0, "sym_inverse": 4.0, "rot_rodrigues": 4.0}
# special values of rcp_ / rsqrt_ outside the contract's domain, as the gfx950 build returns them (hardware estimate +
# Newton steps: 0 * inf in the first step turns 0, denormals and inf into NaN).  The host twin divides (IEEE inf and 0
# there): the call sites that can pass 0 (distance / wheel constraints: rsqrt_(dot(x, x))) multiply by x = 0, NaN both ways
SPECIAL = {"rcp": {0.0: np.nan, -0.0: np.nan, np.inf: np.nan, -np.inf: np.nan, 5e-324: np.nan},
           "rsqrt": {0.0: np.nan, -0.0: np.nan, np.inf: np.nan}}
# (op, precision) pairs the gfx950 build and the host twin compute bit for bit (same operations in the same order);
# the others agree within their contract / faithfulness bounds
# (measured on the fixture's inputs; NaNs compare as NaN).  Not bit for bit: sincos_ f64 (hipcc contracts
# `1 - (0.5 z - z pc)` into an fma: 3 of the 129 145 inputs differ by 1 ulp), rcp_ / rsqrt_ f64 (estimate + Newton steps
# against a division), and the composites whose sums of products hipcc contracts (-ffp-contract=fast, the host build has it off)
BIT_EXACT = {("tanh", "f64"), ("sqrt", "f64"), ("rcp", "f32"), ("rsqrt", "f32"), ("sqrt", "f32"), ("log3", "f32"),
             ("matrix_to_quat", "f64"), ("matrix_to_quat", "f32")}


@pytest.fixture(scope="module")
def fix():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def case(fix, op, tag):
    """inputs, truth (hi, lo) and the reference's float64 value (composites) of one primitive; sincos f64 includes the
    doubles next to k pi/2."""
    x, hi, lo = fix[f"{op}_{tag}_x"], fix[f"{op}_{tag}_hi"], fix[f"{op}_{tag}_lo"]
    if op == "sincos" and tag == "f64":
        k, xk = R.kgrid_inputs(fix)
        sh, sl, ch, cl = R.kgrid_truth(k, xk)
        x = np.concatenate([x, xk[:, None]])
        hi = np.concatenate([hi, np.stack([sh, ch], 1)])
        lo = np.concatenate([lo, np.stack([sl, cl], 1)])
    return x, hi, lo, fix.get(f"{op}_{tag}_ref")


def host_run(op, x, dtype, mode="all"):
    return probe.host(op, x, dtype, mode)


def device_run(op, x, dtype, mode="all"):
    return probe.device(op, x, dtype, mode)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _at_threshold(op, x, dtype):
    """rows whose branch-deciding quantity lies within rounding (a few ulps of `dtype`) of its threshold"""
    rel = 1e-12 if dtype == np.float64 else 1e-5
    near = lambda q, t: np.abs(q / t - 1) < rel
    thr = R.TAYLOR[dtype]
    if op == "exp6":
        return near(np.sqrt((x[:, 3:6] ** 2).sum(1)), thr)
    if op == "quat_exp3":
        return near((x ** 2).sum(1), thr)
    if op == "quat_log3":
        return near((x[:, :3] ** 2).sum(1), thr)
    if op == "jlog3_mul":
        return near(x[:, 0], thr)
    if op == "log3":
        th = np.arccos(np.clip((x[:, 0] + x[:, 4] + x[:, 8] - 1) / 2, -1, 1))
        return near(th, np.pi - R.LOG3_PI_MARGIN) | near(th, thr)
    return np.zeros(len(x), bool)


def _cofactor_error_bound(x, inv, dtype):
    """eps * (|products of each cofactor| / |det| + |inverse entry| * |products of det| / |det|), per entry"""
    xx, xy, xz, yy, yz, zz = x.T
    m = np.stack([np.abs(yy * zz) + yz * yz, np.abs(xz * yz) + np.abs(xy * zz), np.abs(xy * yz) + np.abs(xz * yy),
                  np.abs(xx * zz) + xz * xz, np.abs(xy * xz) + np.abs(xx * yz), np.abs(xx * yy) + xy * xy], 1)
    det = np.abs(xx * (yy * zz - yz * yz) + xy * (xz * yz - xy * zz) + xz * (xy * yz - xz * yy))
    D = np.abs(xx) * m[:, 0] + np.abs(xy) * m[:, 1] + np.abs(xz) * m[:, 2]
    return np.finfo(dtype).eps * (m + np.abs(inv) * D[:, None]) / det[:, None]


def _same(a, b):
    """bit for bit, NaNs compared as NaN"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


# ---- checks, shared by the host twin (CPU leg) and the gfx950 build (gpu leg); each returns the measured maxima
def check_contract(run, fix, op, tag):
    dtype = TAGS[tag]
    x, hi, lo, _ = case(fix, op, tag)
    got = run(op, x, dtype).astype(np.float64)
    xx = x[:, 0].astype(np.float64)
    dom = DOMAIN[op](xx, tag)
    err = R.ulp_err(got[dom], hi[dom], lo[dom], dtype)
    worst = float(err.max())
    bound = HOST_CONTRACT.get((op, tag), CONTRACT[(op, tag)]) if run is host_run else CONTRACT[(op, tag)]
    i = np.unravel_index(int(err.argmax()), err.shape)
    assert worst <= bound, f"{op} {tag}: {worst:.3f} ulp at x = {xx[dom][i[0]]!r} (got {got[dom][i]!r})"
    # outside the domain: sincos_ f64 gives NaN; elsewhere the value is pinned bit for bit below
    if op == "sincos" and tag == "f64":
        assert np.isnan(got[~dom]).all(), xx[~dom][~np.isnan(got[~dom]).all(1)]
    # special values, signs of zero included: exact where the truth is representable
    spec = np.isfinite(xx) & (np.isfinite(hi).all(1)) & (lo == 0).all(1) & ((xx == 0) | (np.abs(xx) < 1e-300)) & dom
    np.testing.assert_array_equal(_bits(got[spec].astype(dtype)), _bits(hi[spec].astype(dtype)), f"{op} {tag} at {xx[spec]}")
    if op in ("sincos", "tanh"):
        nf = ~np.isfinite(xx)
        want = {"sincos": lambda v: np.full(2, np.nan), "tanh": lambda v: np.array([np.copysign(1.0, v) if np.isinf(v) else np.nan])}[op]
        for v, g in zip(xx[nf], got[nf]):
            np.testing.assert_array_equal(g, want(v), f"{op} {tag} at {v}")
    if op in SPECIAL and tag == "f64" and run is device_run:
        for v, w in SPECIAL[op].items():
            sel = _bits(xx) == _bits(np.array([v]))[0]
            assert sel.any(), v
            assert np.all(np.isnan(got[sel]) if np.isnan(w) else got[sel] == w), (op, v, got[sel])
    return worst


def check_faithful(run, fix, op, tag):
    dtype = TAGS[tag]
    x, hi, lo, ref = case(fix, op, tag)
    got = run(op, x, dtype).astype(np.float64)
    ref = ref.reshape(got.shape)
    # the reference's formula in the probe's own precision (float32: evaluated here in float32, with float32 thresholds)
    if tag == "f32":
        ref, branch = R.ref32(op, x)
    else:
        branch = [R.COMPOSITES[op](R.REF, [float(v) for v in row], dtype)[1] for row in x]
    # rows where that formula overflows (jlog3_mul at theta = 2 pi: 1 - cos = 0) stay non-finite; every other row is finite
    finite = np.isfinite(hi).all(1) & np.isfinite(ref).all(1)
    assert not np.isfinite(got[~finite]).all(1).any(), f"{op} {tag}: finite where the reference's formula is not"
    bad = ~np.isfinite(got[finite]).all(1)
    assert not bad.any(), f"{op} {tag}: non-finite output at {x[finite][bad][:4]}"
    # inputs within rounding of a branch threshold may take either branch (a contracted sum of squares moves the
    # decision by an ulp): there the other branch of the reference's formula is accepted as well
    alt = ref.copy()
    F = R.REF32 if tag == "f32" else R.REF
    with np.errstate(all="ignore"):
        for i in np.where(_at_threshold(op, x.astype(np.float64), dtype))[0]:
            row = [F.num(v) for v in x[i]]
            alt[i] = [float(v) for v in R.COMPOSITES[op](F, row, dtype, not branch[i])[0]]
    # sym_inverse: the unit is the first-order error bound of the cofactor formula instead (its cancellation grows with the
    # condition number, up to 1e10 in the fixture)
    unit = _cofactor_error_bound(x.astype(np.float64), hi, dtype) if op == "sym_inverse" else None
    # exp6: an ulp of t = |w| (a contracted dot(w, w) on the device) moves sin t and cos t by t ulps
    arg = np.maximum(1.0, np.sqrt((x[:, 3:6].astype(np.float64) ** 2).sum(1)))[:, None] if op == "exp6" else np.ones((len(x), 1))
    worst = 0.0
    for a, b in R.GROUPS[op]:
        g, h, l, r, r2 = got[finite, a:b], hi[finite, a:b], lo[finite, a:b], ref[finite, a:b], alt[finite, a:b]
        u = R.ulp(np.abs(h).max(1, keepdims=True), dtype)
        u = u if unit is None else np.maximum(u, unit[finite, a:b])
        e_truth = np.abs((g - h) - l) / u
        e_ref = np.minimum(np.abs(g - r), np.abs(g - r2)) / u / arg[finite]
        i = np.unravel_index(int(e_ref.argmax()), e_ref.shape)
        bound = FAITH_REF_OP.get(op, FAITH_REF) if tag == "f64" else F32_REF.get(op, FAITH_REF)
        assert e_ref.max() <= bound, f"{op} {tag}[{a}:{b}]: {e_ref.max():.2f} ulp from the reference's formula at {x[finite][i[0]]}"
        worst = max(worst, float(e_ref.max()))
        if tag == "f64":
            ref_truth = np.maximum(np.abs((r - h) - l), np.abs((r2 - h) - l)) / u
            over = e_truth - ref_truth
            j = np.unravel_index(int(over.argmax()), over.shape)
            assert over.max() <= FAITH_TRUTH, f"{op} {tag}[{a}:{b}]: {over.max():.2f} ulp farther from the truth than the reference at {x[finite][j[0]]}"
        else:
            j = np.unravel_index(int(e_truth.argmax()), e_truth.shape)
            assert e_truth.max() <= F32_TRUTH[op], f"{op} {tag}[{a}:{b}]: {e_truth.max():.2f} float ulp at {x[finite][j[0]]}"
    return worst


def check_properties(run):
    # exp6: R orthonormal; log3(exp6(w)) = w away from pi; quat_exp3 and matrix_to_quat give unit quaternions
    rng = np.random.default_rng(3)
    w = rng.normal(size=(512, 3)) * rng.choice([1e-6, 1e-3, 0.1, 1.0], size=(512, 1))
    w *= np.minimum(1.0, 2.5 / np.linalg.norm(w, axis=1))[:, None]
    M = run("exp6", np.concatenate([rng.normal(size=(512, 3)), w], 1), np.float64)
    Rm = M[:, :9].reshape(-1, 3, 3)
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() <= 1.5e-15     # (R R^T itself rounds: ~5 ulp of 1)
    back = run("log3", M[:, :9], np.float64)
    assert np.abs(back - w).max() <= 1e-14
    q = run("quat_exp3", w, np.float64)
    t2 = np.einsum("ij,ij->i", w, w)   # (the Taylor branch of quaternion::exp3 stops at t2: |q|^2 = 1 - t2^2 / 192 there)
    assert (np.abs(np.einsum("ij,ij->i", q, q) - 1) <= 4.5e-16 + np.where(t2 <= R.TAYLOR[np.float64], t2 * t2 / 192, 0)).all()
    q = run("matrix_to_quat", M[:, :9], np.float64)
    assert np.abs(np.einsum("ij,ij->i", q, q) - 1).max() <= 1e-15
    # sign conventions at pi: a half turn about +axis comes back as +pi axis (log3) and as +axis (matrix_to_quat)
    for axis in np.eye(3):
        Rp = run("exp6", np.concatenate([[0, 0, 0], np.pi * axis])[None], np.float64)[:, :9]
        np.testing.assert_allclose(run("log3", Rp, np.float64)[0], np.pi * axis, atol=1e-7)
        np.testing.assert_allclose(run("matrix_to_quat", Rp, np.float64)[0], np.append(axis, 0.0), atol=1e-15)


# ---- CPU leg: the host twin
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("op", SCALARS)
def test_host_contract(fix, op, tag):
    check_contract(host_run, fix, op, tag)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("op", R.COMPOSITES)
def test_host_faithful(fix, op, tag):
    check_faithful(host_run, fix, op, tag)


def test_host_properties():
    check_properties(host_run)


def test_host_modes(fix):
    for op in probe.OPS:
        x = fix[f"{op}_f64_x"]
        a, d = host_run(op, x, np.float64), host_run(op, x, np.float64, "divergent")
        skip = np.arange(len(x)) % 3 == 1
        assert (_bits(d[skip]) == probe.SENTINEL[np.float64]).all()
        np.testing.assert_array_equal(_bits(a[~skip]), _bits(d[~skip]))


def test_fixture_regenerates_with_mpmath(fix):
    """A subsample of the fixture recomputed with mpmath (the whole file: tools/make_device_math_fixtures.py --check)."""
    mpmath = pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("mkfix", os.path.join(os.path.dirname(os.path.dirname(FIXTURE)), "..", "tools",
                                                                        "make_device_math_fixtures.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    mp = R.mp_system(60)
    rng = np.random.default_rng(7)
    for tag in TAGS:
        for op in SCALARS:
            x = fix[f"{op}_{tag}_x"][:, 0]
            for i in rng.choice(len(x), 12, replace=False):
                want = [mk._to_dd(mpmath, v) for v in mk.scalar_truth(mpmath, op, x[i])]
                np.testing.assert_array_equal([h for h, _ in want], fix[f"{op}_{tag}_hi"][i])
                np.testing.assert_array_equal([l for _, l in want], fix[f"{op}_{tag}_lo"][i])
        for op, fn in R.COMPOSITES.items():
            x = fix[f"{op}_{tag}_x"]
            for i in rng.choice(len(x), 4, replace=False):
                row = [float(v) for v in x[i]]
                ref, br = fn(R.REF, row, TAGS[tag])
                t, _ = fn(mp, row, TAGS[tag], br)
                np.testing.assert_array_equal(ref, fix[f"{op}_{tag}_ref"][i])
                np.testing.assert_array_equal([mk._to_dd(mpmath, mpmath.mpf(v))[0] for v in t], fix[f"{op}_{tag}_hi"][i])
    # the k pi/2 grid: the stored doubles straddle k pi/2, and the exact-arithmetic truth agrees with mpmath
    k, xk = R.kgrid_inputs(fix)
    sh, sl, ch, cl = R.kgrid_truth(k, xk)
    n = len(k) // 2
    for i in np.concatenate([rng.choice(n, 40, replace=False), [0, n - 1]]):
        t = k[i] * mpmath.pi / 2
        assert mpmath.mpf(xk[i]) < t < mpmath.mpf(xk[i + n])
        for j in (i, i + n):
            s, c = mpmath.sin(mpmath.mpf(xk[j])), mpmath.cos(mpmath.mpf(xk[j]))
            assert abs((mpmath.mpf(sh[j]) + sl[j]) - s) <= abs(s) * 2.0 ** -70
            assert abs((mpmath.mpf(ch[j]) + cl[j]) - c) <= abs(c) * 2.0 ** -70


# ---- gpu leg: the gfx950 build
@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("op", SCALARS)
def test_device_contract(gpu_device, fix, op, tag):
    print(f"{op} {tag}: {check_contract(device_run, fix, op, tag):.3f} ulp")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("op", R.COMPOSITES)
def test_device_faithful(gpu_device, fix, op, tag):
    print(f"{op} {tag}: {check_faithful(device_run, fix, op, tag):.3f} ulp")


@pytest.mark.gpu
def test_device_properties(gpu_device):
    check_properties(device_run)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_device_modes_and_host_twin(gpu_device, fix, tag):
    dtype = TAGS[tag]
    for op in probe.OPS:
        x = case(fix, op, tag)[0]
        full = device_run(op, x, dtype)
        div = device_run(op, x, dtype, "divergent")
        skip = np.arange(len(x)) % 3 == 1
        assert (_bits(div[skip]) == probe.SENTINEL[dtype]).all(), f"{op} {tag}: a skipped lane wrote its output"
        np.testing.assert_array_equal(_bits(div[~skip]), _bits(full[~skip]), f"{op} {tag}: divergent lanes")
        n = len(x) if len(x) % 64 else len(x) - 13
        rag = device_run(op, x[:n], dtype, "ragged")
        np.testing.assert_array_equal(_bits(rag), _bits(full[:n]), f"{op} {tag}: ragged length {n}")
        host = host_run(op, x, dtype)
        same = _same(full, host)
        if (op, tag) in BIT_EXACT:
            assert same.all(), f"{op} {tag}: device vs host twin at {x[~same.all(1)][:4]}"
        elif op in SCALARS:
            # the two builds within the sum of their contracts of each other (specials of rcp_ / rsqrt_: SPECIAL)
            dom = DOMAIN[op](x[:, 0].astype(np.float64), tag)
            d = np.abs(full[dom].astype(np.float64) - host[dom]) / R.ulp(host[dom], dtype)
            assert (d[np.isfinite(host[dom])] <= 2 * CONTRACT[(op, tag)]).all(), f"{op} {tag}: device vs host twin"
        print(f"{op} {tag}: device == host twin on {same.all(1).mean():.4f} of the inputs")
