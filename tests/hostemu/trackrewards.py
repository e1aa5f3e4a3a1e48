"""Build + ctypes driver of trackrewards.cpp: the kernel body of the tracking rewards block on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen, trackrewards
from tests import trackrewards_numpy as rn
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_trackrewards.so")
    deps = [os.path.join(_HERE, "trackrewards.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_trackrewards.h", "jm_locomotion.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "trackrewards.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.TrackRewardsDesc)
    L.emu_trackrewards_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_tracking_rewards.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.TrackRewardsIO), C.POINTER(C.c_double), C.c_char_p,
                                       C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: dict):
    """`jm_trackrewards_desc` of a fixture plan (tests/trackrewards_numpy.py names its keys)."""
    return trackrewards.make_desc(**{k: plan[k] for k in rn.PLAN_KEYS})


def pack(desc) -> None:
    """The description check of `jm_trackrewards_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_trackrewards_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_trackrewards_pack failed with code {rc}")


def run(plan: dict, inputs: Dict[str, np.ndarray], cutoff: Sequence[Optional[float]], dtype=np.float64, mask=None,
        into: Optional[Dict[str, np.ndarray]] = None, outputs: Sequence[str] = rn.OUTPUTS) -> Dict[str, np.ndarray]:
    """`trackrewards_lane` on the lanes of `mask` (all without one); inputs that are missing are null pointers, the named
    outputs are written into `into` (default: new arrays of zeros) and returned."""
    desc, keep = plan_desc(plan)
    B = next(iter(inputs.values())).shape[-1]
    io = _abi.TrackRewardsIO()
    held = []
    for name in rn.INPUTS:
        if name in inputs:
            held.append(np.ascontiguousarray(inputs[name], dtype=dtype))
            setattr(io, name, held[-1].ctypes.data)
    if mask is not None:
        held.append(np.ascontiguousarray(mask, dtype=np.uint8))
        io.lane_mask = held[-1].ctypes.data
    out = {}
    for name in outputs:
        a = into[name] if into is not None else np.zeros((rn.rows_of(name, plan), B), dtype=dtype)
        assert a.shape == (rn.rows_of(name, plan), B) and a.dtype == np.dtype(dtype) and a.flags.c_contiguous
        out[name] = a
        setattr(io, name, a.ctypes.data)
    c = (C.c_double * 4)(*[float(x) if x is not None else 0.0 for x in cutoff])
    err = C.create_string_buffer(512)
    rc = _lib().emu_tracking_rewards(C.byref(desc), _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, C.byref(io), c,
                                     err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_tracking_rewards failed with code {rc}")
    del keep
    return out
