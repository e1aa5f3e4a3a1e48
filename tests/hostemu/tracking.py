"""Build + ctypes driver of tracking.cpp: the kernel body of the tracking windows block on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.tracking import make_desc
from tests.hostemu import emu
from tests.tracking_numpy import INPUTS, OUTPUTS, PLAN_KEYS, dtype_of, shape, state_names

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_tracking.so")
    deps = [os.path.join(_HERE, "tracking.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_tracking.h", "jm_locomotion.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "tracking.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.TrackingDesc)
    L.emu_tracking_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_tracking.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.TrackingIO), C.c_int, C.c_double, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict):
    """`jm_tracking_desc` of a plan dictionary (tests/tracking_numpy.py)."""
    return make_desc(**{k: plan[k] for k in PLAN_KEYS})


def pack(desc) -> None:
    """The description check of `jm_tracking_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_tracking_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_tracking_pack failed with code {rc}")


def run(plan: Dict, inputs: Dict[str, np.ndarray], state: Dict[str, np.ndarray], mode: int, mask=None, dtype=np.float64,
        outputs: Sequence[str] = OUTPUTS, into: Optional[Dict[str, np.ndarray]] = None, odometry_cutoff=None,
        B: Optional[int] = None) -> Dict[str, np.ndarray]:
    """`tracking_lane` on the lanes of `mask` (all without one).  `state`: the arrays of `state_names(plan)` that are passed
    (a missing one is a null pointer), updated in place; so with the inputs.  Returns the named outputs, written into the
    arrays of `into` where given (else into arrays filled with NaN)."""
    dtype = np.dtype(dtype)
    B = int(B if B is not None else next(iter(state.values())).shape[-1])
    desc, _ = plan_desc(plan)
    io = _abi.TrackingIO()
    held = []
    for name in INPUTS:
        if name in inputs:
            a = np.ascontiguousarray(inputs[name], dtype=dtype)
            assert a.shape == shape(name, plan, B)
            held.append(a)
            setattr(io, name, a.ctypes.data)
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        held.append(m)
        io.lane_mask = m.ctypes.data
    for name in state_names(plan):
        if name in state:
            a = state[name]
            assert a.shape == shape(name, plan, B) and a.dtype == dtype_of(name, dtype) and a.flags.c_contiguous
            setattr(io, name, a.ctypes.data)
    out = {}
    for name in outputs:
        a = into[name] if into is not None and name in into else np.full(shape(name, plan, B), np.nan, dtype=dtype)
        assert a.shape == shape(name, plan, B) and a.dtype == dtype and a.flags.c_contiguous
        out[name] = a
        setattr(io, name, a.ctypes.data)
    err = C.create_string_buffer(512)
    cutoff = float(plan["odometry_cutoff"] if odometry_cutoff is None else odometry_cutoff)
    rc = _lib().emu_tracking(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io), int(mode), cutoff,
                             err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_tracking failed with code {rc}")
    del held
    return out
