"""Build + ctypes driver of actuation.cpp: the kernel body of the actuated-joint quantities block on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.actuation import make_desc
from tests.actuation_numpy import INPUTS, OUTPUTS, PLAN_KEYS, STATE, output_dtype, output_shape
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_actuation.so")
    deps = [os.path.join(_HERE, "actuation.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_actuation.h", "jm_locomotion.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "actuation.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.ActuationDesc)
    L.emu_actuation_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_actuation.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.ActuationIO), C.c_int, C.c_int, C.c_double, C.c_double,
                                C.c_double, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict):
    """`jm_actuation_desc` of a plan dictionary (tests/actuation_numpy.py) and what keeps its arrays alive."""
    return make_desc(**{k: plan[k] for k in PLAN_KEYS})


def pack(desc) -> None:
    """The description check of `jm_actuation_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_actuation_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_actuation_pack failed with code {rc}")


def launch_scalars(plan: Dict, motor_side=None, position_margin=None, velocity_max=None, power_cutoff=None):
    """The launch scalars of a case, each replaced by the argument where one is given."""
    pick = lambda given, key: plan[key] if given is None else given      # noqa: E731
    return (int(bool(pick(motor_side, "motor_side"))), float(pick(position_margin, "position_margin")),
            float(pick(velocity_max, "velocity_max")), float(pick(power_cutoff, "power_cutoff")))


def run(plan: Dict, inputs: Dict[str, np.ndarray], state: Optional[Dict[str, np.ndarray]], mode: int, mask=None, dtype=np.float64,
        outputs: Sequence[str] = OUTPUTS, into: Optional[Dict[str, np.ndarray]] = None, **scalars) -> Dict[str, np.ndarray]:
    """`actuation_lane` on the lanes of `mask` (all without one).  `state`: `power_ring` and `power_count`, updated in place
    (None: no window).  Returns the named outputs, written into the arrays of `into` where given (else into arrays filled
    with a sentinel: NaN, -1 for the safety count)."""
    dtype = np.dtype(dtype)
    B = next(iter(inputs.values())).shape[-1]
    desc, keep = plan_desc(plan)
    io = _abi.ActuationIO()
    held = [keep]
    for name in INPUTS:
        if name in inputs:
            a = np.ascontiguousarray(inputs[name], dtype=dtype)
            held.append(a)
            setattr(io, name, a.ctypes.data)
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        held.append(m)
        io.lane_mask = m.ctypes.data
    for name in STATE:
        if state is not None:
            a = state[name]
            assert a.shape == output_shape(name, plan, B) and a.dtype == output_dtype(name, dtype) and a.flags.c_contiguous
            setattr(io, name, a.ctypes.data)
    out = {}
    for name in outputs:
        if into is not None and name in into:
            a = into[name]
        else:
            a = np.full(output_shape(name, plan, B), -1 if name == "safety" else np.nan, dtype=output_dtype(name, dtype))
        assert a.shape == output_shape(name, plan, B) and a.dtype == output_dtype(name, dtype) and a.flags.c_contiguous
        out[name] = a
        setattr(io, name, a.ctypes.data)
    err = C.create_string_buffer(512)
    rc = _lib().emu_actuation(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io), int(mode),
                              *launch_scalars(plan, **scalars), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_actuation failed with code {rc}")
    del held
    return out
