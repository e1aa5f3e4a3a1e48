"""Build + ctypes driver of force_process.cpp: the spline of the process forces and the variation instantiations of the
step kernels with process forces in their arguments, on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.model import CompiledModel
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE: Dict[str, C.CDLL] = {}


class EmuProcess(C.Structure):
    _fields_ = [("row", C.c_int), ("n_knots", C.c_int), ("knot_spacing", C.c_double), ("scale", C.c_double),
                ("values", C.c_void_p), ("grads", C.c_void_p)]


def _lib(model: CompiledModel) -> C.CDLL:
    h = model.topology_hash()
    if h in _CACHE:
        return _CACHE[h]
    hdr = codegen.write_header(model)
    out = os.path.join(codegen.BUILD, f"libemu_force_process_{h}.so")
    deps = [os.path.join(_HERE, "force_process.cpp"), os.path.join(_HERE, "emu.cpp"), hdr] + codegen._sources()[1:]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [f"-DJM_TOPO_HEADER=\"{hdr}\"", os.path.join(_HERE, "force_process.cpp"),
                                                     "-o", out])
    L = C.CDLL(out)
    L.emu_process_value.argtypes = [C.POINTER(EmuProcess), C.c_longlong, C.c_longlong, C.c_double]
    L.emu_process_value.restype = C.c_double
    L.emu_run_process.argtypes = [C.POINTER(_abi.ModelDesc), C.POINTER(_abi.Options), C.POINTER(emu.EmuIO), C.c_int, C.c_int,
                                  C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(EmuProcess),
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.emu_set_constraints.argtypes = [C.POINTER(_abi.ConstraintOptions), C.c_void_p, C.c_void_p]
    L.emu_set_constraints.restype = None
    for name in ("emu_set_ground_offset", "emu_set_friction", "emu_set_flexibility"):
        getattr(L, name).argtypes = [C.c_void_p]
        getattr(L, name).restype = None
    L.emu_set_gen.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.emu_set_gen.restype = None
    _CACHE[h] = L
    return L


class Process:
    """One process force of a launch: `row` = 6 * frame + component; `values`, `grads` `[n][B]` float64 (kept alive here)."""

    def __init__(self, row: int, knot_spacing: float, scale: float, values: np.ndarray, grads: np.ndarray) -> None:
        self.row, self.h, self.scale = int(row), float(knot_spacing), float(scale)
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.grads = np.ascontiguousarray(grads, dtype=np.float64)
        assert self.values.shape == self.grads.shape and self.values.ndim == 2

    def struct(self) -> EmuProcess:
        return EmuProcess(self.row, self.values.shape[0], self.h, self.scale, self.values.ctypes.data, self.grads.ctypes.data)


def value(model: CompiledModel, process: Process, lane: int, t: float) -> float:
    """`process_force_value` (jm_kernels.h) of one lane at one time."""
    s = process.struct()
    return float(_lib(model).emu_process_value(C.byref(s), process.values.shape[1], int(lane), float(t)))


def run(model: CompiledModel, arrays: Dict[str, np.ndarray], mode: str, lane_time: np.ndarray, processes: Sequence[Process],
        frames, held: Optional[np.ndarray] = None, constraint_options: Optional[dict] = None, options=None,
        solver: str = "runge_kutta_4", dt: float = 1e-3, n_substeps: int = 1, command_changed: bool = False,
        update_sensors: bool = True, variant: str = "lane") -> None:
    """One launch of the variation code with `processes` registered, float64.  `frames` = (offsets [K][3], parent joints [K]);
    `held` `[6 K][B]` = the held wrenches (None: the rows are not bound); `lane_time` `[1][B]` float64, read and written."""
    L = _lib(model)
    offs = np.ascontiguousarray(frames[0], dtype=np.float64)
    joints = np.ascontiguousarray(frames[1], dtype=np.int32)
    hw = None if held is None else np.ascontiguousarray(held, dtype=np.float64)
    L.emu_set_gen(None, None, 0, 0, 0.0, 0.0, 1.0, 1.0, None, 0, None, None)
    if constraint_options is not None:
        co = _abi.make_constraint_options(**constraint_options)
        L.emu_set_constraints(C.byref(co), arrays["con_flags"].ctypes.data, arrays["con_data"].ctypes.data)
    else:
        co = _abi.make_constraint_options(model="spring_damper")
        L.emu_set_constraints(C.byref(co), None, None)
    L.emu_set_ground_offset(None)
    fr = arrays.get("friction")
    L.emu_set_friction(fr.ctypes.data if fr is not None else None)
    fx = arrays.get("flexibility")
    L.emu_set_flexibility(fx.ctypes.data if fx is not None else None)
    desc, keep = _abi.make_model_desc(model)
    opts = options if options is not None else _abi.make_options()
    io = emu.EmuIO()
    io.B = arrays["q"].shape[-1]
    for n in emu._FIELDS:
        a = arrays.get(n)
        if a is not None:
            assert a.flags.c_contiguous and a.dtype != np.float32, n
            setattr(io, n, a.ctypes.data)
    assert lane_time.dtype == np.float64 and lane_time.flags.c_contiguous and lane_time.size == io.B
    ps = (EmuProcess * max(len(processes), 1))(*[p.struct() for p in processes])
    rc = L.emu_run_process(C.byref(desc), C.byref(opts), C.byref(io), 1 if variant == "quad" else 0, emu.MODES[mode],
                           emu.SOLVERS[solver], float(dt), int(n_substeps), int(command_changed), int(update_sensors),
                           lane_time.ctypes.data, len(processes), ps, None if hw is None else hw.ctypes.data,
                           offs.shape[0], offs.ctypes.data, joints.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"emu_run_process failed with code {rc}")
