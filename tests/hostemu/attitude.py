"""Build + ctypes driver of attitude.cpp: the attitude-observer kernel bodies and the plain Mahony function on the host
(tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

from jiminy_amd import _abi, codegen
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_attitude.so")
    deps = [os.path.join(_HERE, "attitude.cpp"), os.path.join(codegen.CSRC, "jm_attitude.h"), os.path.join(codegen.CSRC, "jm_rotation.h"),
            os.path.join(codegen.CSRC, "jm_math.h"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "attitude.cpp"), "-o", out])
    L = C.CDLL(out)
    vp, desc = C.c_void_p, C.POINTER(_abi.AttitudeDesc)
    L.emu_attitude_init.argtypes = [desc, C.c_int, C.c_longlong, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.emu_mahony_observer.argtypes = [desc, C.c_int, C.c_longlong, vp, vp, vp, vp, vp, C.c_double, C.c_int, vp, C.c_char_p, C.c_size_t]
    L.emu_body_observer.argtypes = [desc, C.c_int, C.c_longlong, vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_double, vp,
                                    C.c_char_p, C.c_size_t]
    L.emu_mahony_filter.argtypes = [C.c_int, C.c_longlong, C.c_int, vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_double]
    _LIB = L
    return L


def _code(dtype) -> int:
    return _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def _raise(rc: int, err, name: str) -> None:
    if rc != 0:
        raise ValueError(err.value.decode() or f"{name} failed with code {rc}")


def init(desc, q, imu, exact_init: bool, quat, omega, cf, bias, twist=None, rpy=None, mask=None) -> None:
    """`attitude_init_lane` on the lanes of `mask` (all without one); the state arrays are updated in place."""
    dtype = quat.dtype
    q, imu = np.ascontiguousarray(q, dtype=dtype), np.ascontiguousarray(imu, dtype=dtype)
    B = quat.shape[-1]
    assert imu.shape == (desc.n_imu, 6, B) and q.shape == (desc.nq, B) and quat.shape == (4, desc.n_imu, B)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    err = C.create_string_buffer(512)
    rc = _lib().emu_attitude_init(C.byref(desc), _code(dtype), B, _ptr(q), _ptr(imu), _ptr(m), int(exact_init), _ptr(quat),
                                  _ptr(omega), _ptr(cf), _ptr(bias), _ptr(twist), _ptr(rpy), err, 512)
    _raise(rc, err, "emu_attitude_init")


def mahony(desc, imu, quat, omega, cf, bias, dt: float, ignore_twist: bool, rpy=None) -> None:
    dtype = quat.dtype
    imu = np.ascontiguousarray(imu, dtype=dtype)
    B = quat.shape[-1]
    assert imu.shape == (desc.n_imu, 6, B) and quat.shape == (4, desc.n_imu, B)
    err = C.create_string_buffer(512)
    rc = _lib().emu_mahony_observer(C.byref(desc), _code(dtype), B, _ptr(imu), _ptr(quat), _ptr(omega), _ptr(cf), _ptr(bias),
                                    float(dt), int(ignore_twist), _ptr(rpy), err, 512)
    _raise(rc, err, "emu_mahony_observer")


def body(desc, imu_quat, imu_omega, quat, omega, twist, twist_mode: int, time_constant_inv: float, dt: float, rpy=None) -> None:
    dtype = quat.dtype
    iq, io = np.ascontiguousarray(imu_quat, dtype=dtype), np.ascontiguousarray(imu_omega, dtype=dtype)
    B = quat.shape[-1]
    assert iq.shape == quat.shape == (4, desc.n_imu, B) and io.shape == (3, desc.n_imu, B)
    err = C.create_string_buffer(512)
    rc = _lib().emu_body_observer(C.byref(desc), _code(dtype), B, _ptr(iq), _ptr(io), _ptr(quat), _ptr(omega), _ptr(twist),
                                  int(twist_mode), float(time_constant_inv), float(dt), _ptr(rpy), err, 512)
    _raise(rc, err, "emu_body_observer")


def mahony_function(imu, quat, omega, cf, bias, kp: float, ki: float, dt: float) -> None:
    """`mahony_lane` with one pair of gains (what `k_mahony` runs); quat, omega, cf, bias are updated in place."""
    dtype = quat.dtype
    imu = np.ascontiguousarray(imu, dtype=dtype)
    n_imu, B = quat.shape[1:]
    assert imu.shape == (n_imu, 6, B) and quat.shape == (4, n_imu, B) and omega.shape == cf.shape == bias.shape == (3, n_imu, B)
    rc = _lib().emu_mahony_filter(_code(dtype), B, n_imu, _ptr(imu), _ptr(quat), _ptr(omega), _ptr(cf), _ptr(bias), float(kp),
                                  float(ki), float(dt))
    if rc != 0:
        raise ValueError(f"emu_mahony_filter failed with code {rc}")
