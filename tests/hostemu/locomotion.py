"""Build + ctypes driver of locomotion.cpp: the kernel body of the locomotion quantities block on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.locomotion import make_desc
from tests.hostemu import emu
from tests.locomotion_numpy import INPUTS, OUTPUTS, output_shape

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None
DESC_KEYS = ("body_mass", "root_inertia", "gravity", "omega", "contact_foot", "contact_column", "n_feet", "n_frames", "root_column",
             "zmp_frame", "dcm_frame")


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_locomotion.so")
    deps = [os.path.join(_HERE, "locomotion.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_locomotion.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "locomotion.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.LocomotionDesc)
    L.emu_locomotion_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_locomotion.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.LocomotionIO), C.c_double, C.c_double, C.c_char_p,
                                 C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict):
    """`jm_locomotion_desc` of a plan dictionary (tests/locomotion_numpy.py) and what keeps its arrays alive."""
    return make_desc(**{k: plan[k] for k in DESC_KEYS})


def pack(desc) -> None:
    """The description check of `jm_locomotion_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_locomotion_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_locomotion_pack failed with code {rc}")


def run(plan: Dict, inputs: Dict[str, np.ndarray], dtype=np.float64, outputs: Sequence[str] = OUTPUTS, mask=None,
        into: Optional[Dict[str, np.ndarray]] = None, momentum_cutoff: Optional[float] = None,
        friction_cutoff: Optional[float] = None) -> Dict[str, np.ndarray]:
    """`locomotion_lane` on the lanes of `mask` (all without one).  Returns the named outputs, written into the arrays of
    `into` where given (else into arrays filled with a sentinel NaN)."""
    dtype = np.dtype(dtype)
    B = inputs["centroidal"].shape[-1] if "centroidal" in inputs else next(iter(inputs.values())).shape[-1]
    desc, keep = plan_desc(plan)
    io = _abi.LocomotionIO()
    held = [keep]
    for name in INPUTS:
        if name in inputs:
            a = np.ascontiguousarray(inputs[name], dtype=np.int32 if name == "con_flags" else dtype)
            held.append(a)
            setattr(io, name, a.ctypes.data)
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        held.append(m)
        io.lane_mask = m.ctypes.data
    out = {}
    for name in outputs:
        a = into[name] if into is not None and name in into else np.full(output_shape(name, plan, B), np.nan, dtype=dtype)
        assert a.shape == output_shape(name, plan, B) and a.dtype == dtype and a.flags.c_contiguous
        out[name] = a
        setattr(io, name, a.ctypes.data)
    err = C.create_string_buffer(512)
    mc = plan["momentum_cutoff"] if momentum_cutoff is None else momentum_cutoff
    fc = plan["friction_cutoff"] if friction_cutoff is None else friction_cutoff
    rc = _lib().emu_locomotion(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io), float(mc), float(fc),
                               err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_locomotion failed with code {rc}")
    del held
    return out
