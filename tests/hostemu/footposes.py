"""Build + ctypes driver of footposes.cpp: the kernel body of the foot pose quantities block on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.footposes import make_desc
from tests.footposes_numpy import INPUTS, OUTPUTS, output_shape
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None
DESC_KEYS = ("foot_column", "n_frames")


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_footposes.so")
    deps = [os.path.join(_HERE, "footposes.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_footposes.h", "jm_locomotion.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "footposes.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.FootPosesDesc)
    L.emu_footposes_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_footposes.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.FootPosesIO), C.c_double, C.c_double, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict):
    """`jm_footposes_desc` of a plan dictionary (tests/footposes_numpy.py) and what keeps its arrays alive."""
    return make_desc(**{k: plan[k] for k in DESC_KEYS})


def pack(desc) -> None:
    """The description check of `jm_footposes_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_footposes_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_footposes_pack failed with code {rc}")


def run(plan: Dict, inputs: Dict[str, np.ndarray], dtype=np.float64, outputs: Sequence[str] = OUTPUTS, mask=None,
        into: Optional[Dict[str, np.ndarray]] = None, position_cutoff: Optional[float] = None,
        orientation_cutoff: Optional[float] = None, fill=np.nan) -> Dict[str, np.ndarray]:
    """`footposes_lane` on the lanes of `mask` (all without one).  Returns the named outputs, written into the arrays of `into`
    where given (else into arrays filled with `fill`)."""
    dtype = np.dtype(dtype)
    B = inputs["pose"].shape[-1]
    desc, keep = plan_desc(plan)
    io = _abi.FootPosesIO()
    held = [keep]
    for name in INPUTS:
        if name in inputs:
            a = np.ascontiguousarray(inputs[name], dtype=dtype)
            held.append(a)
            setattr(io, name, a.ctypes.data if a.size else None)
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        held.append(m)
        io.lane_mask = m.ctypes.data
    out = {}
    for name in outputs:
        a = into[name] if into is not None and name in into else np.full(output_shape(name, plan, B), fill, dtype=dtype)
        assert a.shape == output_shape(name, plan, B) and a.dtype == dtype and a.flags.c_contiguous
        out[name] = a
        setattr(io, name, a.ctypes.data if a.size else None)
    err = C.create_string_buffer(512)
    pc = plan["position_cutoff"] if position_cutoff is None else position_cutoff
    oc = plan["orientation_cutoff"] if orientation_cutoff is None else orientation_cutoff
    rc = _lib().emu_footposes(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io), float(pc), float(oc),
                              err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_footposes failed with code {rc}")
    del held
    return out
