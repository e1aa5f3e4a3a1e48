"""Build + ctypes driver of lane_ground.cpp: the one-robot-per-lane constraint kernel (variation instantiation) on a
height-map ground, on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.model import CompiledModel
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE: Dict[str, C.CDLL] = {}


def _lib(model: CompiledModel) -> C.CDLL:
    h = model.topology_hash()
    if h in _CACHE:
        return _CACHE[h]
    hdr = codegen.write_header(model)
    out = os.path.join(codegen.BUILD, f"libemu_lane_ground_{h}.so")
    deps = [os.path.join(_HERE, "lane_ground.cpp"), os.path.join(_HERE, "emu.cpp"), hdr] + codegen._sources()[1:]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [f"-DJM_TOPO_HEADER=\"{hdr}\"", os.path.join(_HERE, "lane_ground.cpp"),
                                                     "-o", out])
    L = C.CDLL(out)
    L.emu_run_lane_ground.argtypes = [C.POINTER(_abi.ModelDesc), C.POINTER(_abi.Options), C.POINTER(emu.EmuIO),
                                      C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int]
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


def run(model: CompiledModel, arrays: Dict[str, np.ndarray], mode: str, constraint_options: dict, ground=None,
        model_lane=None, options=None, solver: str = "runge_kutta_4", dt: float = 1e-3, n_substeps: int = 1,
        command_changed: bool = True, update_sensors: bool = True) -> None:
    """One launch of `k_constrained<double, Topo, true>`'s code on the host, float64.  `ground` = (heights [ny][nx], x0, y0,
    dx, dy) or None (flat ground through the same instantiation); `arrays["ground_offset"]` `[2][B]`: every lane's patch;
    `arrays["con_flags"]` / `["con_data"]`: the constraint state (tests.helpers.alloc_constraint_state)."""
    L = _lib(model)
    gh = None if ground is None else np.ascontiguousarray(ground[0], dtype=np.float64)
    g = ground if ground is not None else (None, 0.0, 0.0, 1.0, 1.0)
    ml = None if model_lane is None else np.ascontiguousarray(model_lane, dtype=np.float64)
    L.emu_set_gen(None if ml is None else ml.ctypes.data, None if gh is None else gh.ctypes.data,
                  0 if gh is None else gh.shape[1], 0 if gh is None else gh.shape[0], float(g[1]), float(g[2]), float(g[3]),
                  float(g[4]), None, 0, None, None)
    co = _abi.make_constraint_options(**constraint_options)
    L.emu_set_constraints(C.byref(co), arrays["con_flags"].ctypes.data, arrays["con_data"].ctypes.data)
    go = arrays.get("ground_offset")
    L.emu_set_ground_offset(go.ctypes.data if (go is not None and gh is not None) else None)
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
    rc = L.emu_run_lane_ground(C.byref(desc), C.byref(opts), C.byref(io), emu.MODES[mode], emu.SOLVERS[solver], float(dt),
                               int(n_substeps), int(command_changed), int(update_sensors))
    if rc != 0:
        raise RuntimeError(f"emu_run_lane_ground failed with code {rc}")
