"""Build + ctypes driver of observe.cpp: the kernel body of the observation assembly on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.observe import make_desc
from tests.hostemu import emu
from tests.observe_numpy import PLAN_KEYS

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_observe.so")
    deps = [os.path.join(_HERE, "observe.cpp"), os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_observe.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [os.path.join(_HERE, "observe.cpp"), "-o", out])
    L = C.CDLL(out)
    desc = C.POINTER(_abi.ObserveDesc)
    L.emu_observe_pack.argtypes = [desc, C.c_char_p, C.c_size_t]
    L.emu_observe.argtypes = [desc, C.c_int, C.c_int, C.c_longlong, C.POINTER(_abi.ObserveIO), C.c_int, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def plan_desc(plan: Dict):
    """`jm_observe_desc` of a plan dictionary (tests/observe_numpy.py) and what keeps its arrays alive."""
    return make_desc(**{k: plan[k] for k in PLAN_KEYS})


def pack(desc) -> None:
    """The description check of `jm_observe_plan_create`; raises ValueError with its message."""
    err = C.create_string_buffer(512)
    rc = _lib().emu_observe_pack(None if desc is None else C.byref(desc), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_observe_pack failed with code {rc}")


def code(dtype) -> int:
    return _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32


def run(plan: Dict, sources: Sequence[np.ndarray], hist: np.ndarray, out: np.ndarray, shift: bool = True,
        reset_mask: Optional[np.ndarray] = None, dtype_in=np.float64, dtype_out=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """One launch on the host: `hist` and `out` are updated in place (and returned); `sources` are used as they are."""
    desc, keep = plan_desc(plan)
    io = _abi.ObserveIO()
    for s, a in enumerate(sources):
        assert a.flags.c_contiguous and a.dtype == np.dtype(dtype_in)
        io.source[s] = a.ctypes.data
    assert hist.flags.c_contiguous and hist.dtype == np.dtype(dtype_in) and out.flags.c_contiguous and out.dtype == np.dtype(dtype_out)
    io.hist, io.out = hist.ctypes.data, out.ctypes.data
    mask = None if reset_mask is None else np.ascontiguousarray(reset_mask, dtype=np.uint8)
    io.reset_mask = None if mask is None else mask.ctypes.data
    err = C.create_string_buffer(512)
    rc = _lib().emu_observe(C.byref(desc), code(dtype_in), code(dtype_out), sources[0].shape[-1], C.byref(io), int(bool(shift)), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_observe failed with code {rc}")
    del keep, mask
    return out, hist
