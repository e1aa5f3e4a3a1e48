"""Build + ctypes driver of deform.cpp: the DeformationEstimator kernel body on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional, Tuple

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
    out = os.path.join(codegen.BUILD, "libemu_deform.so")
    deps = [os.path.join(_HERE, "deform.cpp"), os.path.join(codegen.CSRC, "jm_deform.h"), os.path.join(codegen.CSRC, "jm_rotation.h"),
            os.path.join(codegen.CSRC, "jm_math.h"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "deform.cpp"), "-o", out])
    L = C.CDLL(out)
    L.emu_deformation_estimator.argtypes = [C.POINTER(_abi.DeformDesc), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def run(desc: "_abi.DeformDesc", encoder: np.ndarray, imu_quat: np.ndarray, compute_rpy: bool = True,
        dtype=np.float64) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """`deform_lane<dtype>` for every lane.  encoder `[n_enc][2][B]`, imu_quat `[4][n_imu][B]` -> quat `[4][n_flex][B]`,
    rpy `[3][n_flex][B]` (None without `compute_rpy`)."""
    enc = np.ascontiguousarray(encoder, dtype=dtype)
    imu = np.ascontiguousarray(imu_quat, dtype=dtype)
    B = imu.shape[-1]
    assert enc.shape == (desc.n_enc, 2, B) and imu.shape == (4, desc.n_imu, B)
    quat = np.full((4, desc.n_flex, B), np.nan, dtype=dtype)
    rpy = np.full((3, desc.n_flex, B), np.nan, dtype=dtype) if compute_rpy else None
    err = C.create_string_buffer(512)
    rc = _lib().emu_deformation_estimator(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B,
                                          enc.ctypes.data, imu.ctypes.data, quat.ctypes.data,
                                          None if rpy is None else rpy.ctypes.data, err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_deformation_estimator failed with code {rc}")
    return quat, rpy
