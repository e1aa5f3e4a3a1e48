"""Build + ctypes driver of trajectory.cpp: the kernel body of the reference trajectories block on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.trajectory import make_desc
from tests.hostemu import emu
from tests.trajectory_numpy import OUTPUTS, PLAN_KEYS, dtype_of, rows_of

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_trajectory.so")
    deps = [os.path.join(_HERE, "trajectory.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_trajectory.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "trajectory.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.TrajectoryDesc)
    L.emu_trajectory_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_trajectory.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.TrajectoryIO), C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict, dtype=np.float64):
    """`jm_trajectory_desc` of a plan dictionary (tests/trajectory_numpy.py) and what keeps its arrays alive."""
    return make_desc(dtype=dtype, **{k: plan.get(k) for k in PLAN_KEYS})


def pack(desc) -> None:
    """The description check of `jm_trajectory_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_trajectory_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_trajectory_pack failed with code {rc}")


def run(plan: Dict, time, trajectory, time_offset, mask=None, dtype=np.float64, outputs: Sequence[str] = OUTPUTS,
        into: Optional[Dict[str, np.ndarray]] = None, absent: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """`trajectory_state_lane` on the lanes of `mask` (all without one).  Returns the named outputs the plan has, written into
    the arrays of `into` where given (else into arrays filled with NaN, status with -1).  `absent`: arrays passed for outputs
    the plan does not have (the kernel must leave them alone)."""
    dtype = np.dtype(dtype)
    time = np.ascontiguousarray(time, dtype=np.float64)
    B = int(time.shape[0])
    desc, keep = plan_desc(plan, dtype)
    io = _abi.TrajectoryIO()
    trajectory = np.ascontiguousarray(trajectory, dtype=np.int32)
    time_offset = np.ascontiguousarray(time_offset, dtype=np.float64)
    assert trajectory.shape == time_offset.shape == (B,)
    io.time, io.trajectory, io.time_offset = time.ctypes.data, trajectory.ctypes.data, time_offset.ctypes.data
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        keep.append(m)
        io.lane_mask = m.ctypes.data
    out = {}
    for name in outputs:
        rows = rows_of(name, plan)
        if not rows:
            continue
        kind = dtype_of(name, dtype)
        a = into[name] if into is not None and name in into else np.full((rows, B), -1 if name == "status" else np.nan, dtype=kind)
        assert a.shape == (rows, B) and a.dtype == kind and a.flags.c_contiguous
        out[name] = a
        setattr(io, name, a.ctypes.data)
    for name, a in (absent or {}).items():
        assert not rows_of(name, plan) and a.flags.c_contiguous
        setattr(io, name, a.ctypes.data)
    err = C.create_string_buffer(512)
    rc = _lib().emu_trajectory(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_trajectory failed with code {rc}")
    del keep
    return out
