"""Build + ctypes driver of locomotion_ground.cpp: `locomotion_lane<T, true>`, the kernel body of the locomotion quantities
block on height-map ground, on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from tests.hostemu import emu
from tests.hostemu.locomotion import plan_desc
from tests.locomotion_ground_numpy import INPUTS, OUTPUTS, output_shape

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB: Optional[C.CDLL] = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_locomotion_ground.so")
    src = os.path.join(_HERE, "locomotion_ground.cpp")
    deps = [src, os.path.join(codegen.CSRC, "..", "..", "include", "jiminy_hip.h")] + \
           [os.path.join(codegen.CSRC, n) for n in ("jm_locomotion.h", "jm_ground.h", "jm_frames.h", "jm_rotation.h", "jm_math.h")]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [src, "-o", out])
    L = C.CDLL(out)
    L.emu_locomotion_ground.argtypes = [C.POINTER(_abi.LocomotionDesc), C.c_int, C.c_longlong, C.POINTER(_abi.LocomotionIO),
                                        C.POINTER(_abi.LocomotionGround), C.c_double, C.c_double, C.c_char_p, C.c_size_t]
    _LIB = L
    return L


def ground_struct(ground: Optional[Dict], dtype, held: list, pointer) -> Optional["_abi.LocomotionGround"]:
    """`jm_locomotion_ground` of a ground dictionary (tests/locomotion_ground_numpy.py); `pointer(array) -> address` places the
    arrays (`held` keeps them alive).  None: no structure."""
    if ground is None:
        return None
    g = _abi.LocomotionGround()
    if ground.get("heights") is not None:
        H = np.ascontiguousarray(ground["heights"], dtype=dtype)
        g.heights, g.ny, g.nx = pointer(H), H.shape[0], H.shape[1]
        g.x0, g.y0, g.dx, g.dy = (float(ground[k]) for k in ("x0", "y0", "dx", "dy"))
    if ground.get("offsets") is not None:
        g.offsets = pointer(np.ascontiguousarray(ground["offsets"], dtype=dtype))
    return g


def run(plan: Dict, inputs: Dict[str, np.ndarray], ground: Optional[Dict], dtype=np.float64, outputs: Sequence[str] = OUTPUTS,
        mask=None, into: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """`locomotion_lane<T, true>` on the lanes of `mask` (all without one).  `ground` None: a null `jm_locomotion_ground`
    (then `contact_ground` cannot be asked for).  Returns the named outputs, written into the arrays of `into` where given
    (else into arrays filled with a sentinel NaN)."""
    dtype = np.dtype(dtype)
    B = inputs["centroidal"].shape[-1]
    desc, keep = plan_desc(plan)
    io = _abi.LocomotionIO()
    held = [keep]

    def pointer(a):
        held.append(a)
        return a.ctypes.data
    for name in INPUTS:
        if name in inputs:
            setattr(io, name, pointer(np.ascontiguousarray(inputs[name], dtype=np.int32 if name == "con_flags" else dtype)))
    if mask is not None:
        io.lane_mask = pointer(np.ascontiguousarray(mask, dtype=np.uint8))
    g = ground_struct(ground, dtype, held, pointer)
    out = {}
    for name in outputs:
        if name == "contact_ground" and g is None:
            continue
        a = into[name] if into is not None and name in into else np.full(output_shape(name, plan, B), np.nan, dtype=dtype)
        assert a.shape == output_shape(name, plan, B) and a.dtype == dtype and a.flags.c_contiguous
        out[name] = a
        if name == "contact_ground":
            g.contact_ground = a.ctypes.data
        else:
            setattr(io, name, a.ctypes.data)
    err = C.create_string_buffer(512)
    rc = _lib().emu_locomotion_ground(C.byref(desc), _abi.JM_F64 if dtype == np.float64 else _abi.JM_F32, B, C.byref(io),
                                      None if g is None else C.byref(g), float(plan["momentum_cutoff"]), float(plan["friction_cutoff"]),
                                      err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"emu_locomotion_ground failed with code {rc}")
    del held
    return out
