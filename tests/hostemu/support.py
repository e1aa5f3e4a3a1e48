"""Build + ctypes driver of support.cpp: the kernel body of the projected support polygon block on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.support import make_desc
from tests.hostemu import emu
from tests.support_numpy import INPUTS, INT_OUTPUTS, OUTPUTS, output_shape

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None
DESC_KEYS = ("point_column", "n_frames", "reference_frame")


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_support.so")
    deps = [os.path.join(_HERE, "support.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_support.h", "jm_locomotion.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "support.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.SupportDesc)
    L.emu_support_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_support.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.SupportIO), C.c_double, C.c_double, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict):
    """`jm_support_desc` of a plan dictionary (tests/support_numpy.py) and what keeps its arrays alive."""
    return make_desc(**{k: plan[k] for k in DESC_KEYS})


def pack(desc) -> None:
    """The description check of `jm_support_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_support_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_support_pack failed with code {rc}")


def new_output(name: str, plan: Dict, B: int, dtype, fill) -> np.ndarray:
    """An output array filled with `fill` (the integer ones with -7 where `fill` is not a number)."""
    if name in INT_OUTPUTS:
        return np.full(output_shape(name, plan, B), -7 if fill != fill else int(fill), dtype=np.int32)
    return np.full(output_shape(name, plan, B), fill, dtype=dtype)


def run(plan: Dict, inputs: Dict[str, np.ndarray], dtype=np.float64, outputs: Sequence[str] = OUTPUTS, mask=None,
        into: Optional[Dict[str, np.ndarray]] = None, cutoff_inner: Optional[float] = None, cutoff_outer: Optional[float] = None,
        fill=np.nan) -> Dict[str, np.ndarray]:
    """`support_lane` on the lanes of `mask` (all without one).  Returns the named outputs, written into the arrays of `into`
    where given (else into arrays filled with `fill`)."""
    dtype = np.dtype(dtype)
    B = inputs["pose"].shape[-1]
    desc, keep = plan_desc(plan)
    io = _abi.SupportIO()
    held = [keep]
    for name in INPUTS:
        if inputs.get(name) is not None:
            a = np.ascontiguousarray(inputs[name], dtype=dtype)
            held.append(a)
            setattr(io, name, a.ctypes.data)
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        held.append(m)
        io.lane_mask = m.ctypes.data
    out = {}
    for name in outputs:
        a = into[name] if into is not None and name in into else new_output(name, plan, B, dtype, fill)
        assert a.shape == output_shape(name, plan, B) and a.flags.c_contiguous
        assert a.dtype == (np.int32 if name in INT_OUTPUTS else dtype)
        out[name] = a
        setattr(io, name, a.ctypes.data)
    err = C.create_string_buffer(512)
    ci = plan.get("cutoff_inner", 0.0) if cutoff_inner is None else cutoff_inner
    co = plan.get("cutoff_outer", 0.0) if cutoff_outer is None else cutoff_outer
    rc = _lib().emu_support(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io), float(ci), float(co),
                            err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_support failed with code {rc}")
    del held
    return out
