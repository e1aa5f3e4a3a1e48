"""Build + ctypes driver of centroidal.cpp: the kernel body of the centroidal state block on the host (tests only)."""
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
    out = os.path.join(codegen.BUILD, "libemu_centroidal.so")
    deps = [os.path.join(_HERE, "centroidal.cpp"), os.path.join(codegen.CSRC, "jm_centroidal.h"), os.path.join(codegen.CSRC, "jm_frames.h"),
            os.path.join(codegen.CSRC, "jm_rotation.h"), os.path.join(codegen.CSRC, "jm_math.h"),
            os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "centroidal.cpp"), "-o", out])
    L = C.CDLL(out)
    vp, desc = C.c_void_p, C.POINTER(_abi.CentroidalDesc)
    L.emu_centroidal_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_centroidal_state.argtypes = [desc, C.c_int, C.c_longlong, vp, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def pack(desc) -> None:
    """The description check of `jm_centroidal_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_centroidal_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_centroidal_pack failed with code {rc}")


def run(desc, q, v, a=None, mask=None, dtype=np.float64, into: Optional[np.ndarray] = None, absent: bool = False) -> Optional[np.ndarray]:
    """`centroidal_lane` on the lanes of `mask` (all without one) in `dtype`; the `[15][B]` result is written into `into`
    (default: a new array of NaN) and returned.  `absent`: the call without its output, which returns None."""
    B = np.asarray(q).shape[-1]
    q = np.ascontiguousarray(q, dtype=dtype)
    v = np.ascontiguousarray(v, dtype=dtype)
    a = None if a is None else np.ascontiguousarray(a, dtype=dtype)
    assert q.shape == (desc.nq, B) and v.shape == (desc.nv, B) and (a is None or a.shape == (desc.nv, B))
    out = None
    if not absent:
        out = np.full((15, B), np.nan, dtype=dtype) if into is None else into
        assert out.shape == (15, B) and out.dtype == np.dtype(dtype) and out.flags.c_contiguous
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    err = C.create_string_buffer(512)
    rc = _lib().emu_centroidal_state(C.byref(desc), _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, _ptr(q), _ptr(v),
                                     _ptr(a), _ptr(m), _ptr(out), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_centroidal_state failed with code {rc}")
    return out
