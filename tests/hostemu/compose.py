"""Build + ctypes driver of compose.cpp: the kernel body of the composition layer on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.compositions import make_desc
from tests.compose_numpy import OUTPUT_DTYPES, OUTPUTS, PLAN_KEYS, cast_sources, output_shape
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_compose.so")
    deps = [os.path.join(_HERE, "compose.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_compose.h", "jm_locomotion.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "compose.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.ComposeDesc)
    L.emu_compose_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_compose.argtypes = [desc, C.c_int, C.c_longlong, C.POINTER(_abi.ComposeIO), C.c_int, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict):
    """`jm_compose_desc` of a plan dictionary (tests/compose_numpy.py) and what keeps its arrays alive."""
    return make_desc(**{k: plan[k] for k in PLAN_KEYS})


def pack(desc) -> None:
    """The description check of `jm_compose_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_compose_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_compose_pack failed with code {rc}")


def new_output(name: str, plan: Dict, B: int, dtype, fill) -> np.ndarray:
    """An output array filled with `fill` (the integer ones with 7 where `fill` is not a whole number)."""
    if name in OUTPUT_DTYPES:
        return np.full(output_shape(name, plan, B), 7 if fill != int(fill) else int(fill), dtype=OUTPUT_DTYPES[name])
    return np.full(output_shape(name, plan, B), fill, dtype=dtype)


def run(plan: Dict, inputs: Dict, dtype=np.float64, outputs: Sequence[str] = OUTPUTS, mask=None,
        into: Optional[Dict[str, np.ndarray]] = None, training: Optional[bool] = None, fill=7.25) -> Dict[str, np.ndarray]:
    """`compose_lane` on the lanes of `mask` (all without one).  Returns the named outputs, written into the arrays of `into`
    where given (else into arrays filled with `fill`)."""
    dtype = np.dtype(dtype)
    sources = cast_sources(plan, inputs["sources"], dtype)
    B = sources[0].shape[-1]
    desc, keep = plan_desc(plan)
    io = _abi.ComposeIO()
    held = [keep, sources]
    for s, a in enumerate(sources):
        io.source[s] = a.ctypes.data
    for name, kind in (("time", dtype), ("base_terminated", np.uint8), ("base_truncated", np.uint8)):
        if inputs.get(name) is not None:
            a = np.ascontiguousarray(inputs[name], dtype=kind)
            held.append(a)
            setattr(io, name, a.ctypes.data)
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        held.append(m)
        io.lane_mask = m.ctypes.data
    out = {}
    for name in outputs:
        a = into[name] if into is not None and name in into else new_output(name, plan, B, dtype, fill)
        assert a.shape == output_shape(name, plan, B) and a.flags.c_contiguous and a.dtype == OUTPUT_DTYPES.get(name, dtype)
        out[name] = a
        setattr(io, name, a.ctypes.data)
    err = C.create_string_buffer(512)
    training = inputs["training"] if training is None else training
    rc = _lib().emu_compose(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io), int(bool(training)), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_compose failed with code {rc}")
    del held
    return out
