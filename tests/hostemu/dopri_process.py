"""Build + ctypes driver of dopri_process.cpp: the persistent adaptive stepper (jm_qdopri.h, variation form) with process
forces in its arguments, on the host (tests only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

from jiminy_amd import _abi, codegen
from jiminy_amd.model import CompiledModel
from tests.hostemu import emu
from tests.hostemu.force_process import EmuProcess, Process

_HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE: Dict[str, C.CDLL] = {}


def _lib(model: CompiledModel) -> C.CDLL:
    h = model.topology_hash()
    if h in _CACHE:
        return _CACHE[h]
    hdr = codegen.write_header(model)
    out = os.path.join(codegen.BUILD, f"libemu_dopri_process_{h}.so")
    deps = [os.path.join(_HERE, n) for n in ("dopri_process.cpp", "force_process.cpp", "emu.cpp")] + [hdr] + codegen._sources()[1:]
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(emu.host_compiler() + [f"-DJM_TOPO_HEADER=\"{hdr}\"", os.path.join(_HERE, "dopri_process.cpp"),
                                                     "-o", out])
    L = C.CDLL(out)
    L.emu_run_dopri_process.argtypes = [C.POINTER(_abi.ModelDesc), C.POINTER(_abi.Options), C.POINTER(emu.EmuIO), C.c_void_p,
                                        C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EmuProcess), C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p]
    _CACHE[h] = L
    return L


def run(model: CompiledModel, arrays: Dict[str, np.ndarray], adaptive: Dict[str, np.ndarray], t_next: float,
        lane_time: np.ndarray, processes: Sequence[Process], frames, held: Optional[np.ndarray] = None, tol_rel: float = 1e-4,
        tol_abs: float = 1e-5, dt_max: float = 0.02, dt_restore_threshold_rel: float = 0.2,
        successive_iter_failed_max: int = 1000, new_step: bool = True, options=None, max_attempts: int = 100000):
    """Every robot of `arrays` to `t_next` through `quad_dopri_run<..., GEN = true>` with `processes` registered.  `adaptive`:
    the per-lane stepper state in the oracle's form (oracle_py.adaptive_state), updated in place; `lane_time` `[1][B]`
    float64, read and written; `frames` = (offsets [K][3], parent joints [K]); `held` `[6 K][B]` or None.  Returns (robots
    still active, largest attempt count)."""
    L = _lib(model)
    B = arrays["q"].shape[-1]
    fs = np.zeros((len(emu._AD_F), B))
    isv = np.zeros((len(emu._AD_I), B), dtype=np.int32)
    for i, n in enumerate(emu._AD_F[:4]):
        fs[i] = adaptive[n]
    for i, n in enumerate(emu._AD_I[:4]):
        isv[i] = adaptive[n]
    offs = np.ascontiguousarray(frames[0], dtype=np.float64)
    joints = np.ascontiguousarray(frames[1], dtype=np.int32)
    hw = None if held is None else np.ascontiguousarray(held, dtype=np.float64)
    desc, keep = _abi.make_model_desc(model)
    opts = options if options is not None else _abi.make_options()
    io = emu.EmuIO()
    io.B = B
    for n in emu._FIELDS:
        a = arrays.get(n)
        if a is not None:
            assert a.flags.c_contiguous and a.dtype != np.float32, n
            setattr(io, n, a.ctypes.data)
    assert lane_time.dtype == np.float64 and lane_time.flags.c_contiguous and lane_time.size == B
    ps = (EmuProcess * max(len(processes), 1))(*[p.struct() for p in processes])
    counters = np.zeros(2, dtype=np.int32)
    rc = L.emu_run_dopri_process(C.byref(desc), C.byref(opts), C.byref(io), fs.ctypes.data, isv.ctypes.data, float(t_next),
                                 float(tol_rel), float(tol_abs), float(dt_max), float(dt_restore_threshold_rel),
                                 int(successive_iter_failed_max), int(new_step), int(max_attempts), counters.ctypes.data,
                                 lane_time.ctypes.data, len(processes), ps, None if hw is None else hw.ctypes.data,
                                 offs.shape[0], offs.ctypes.data, joints.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"emu_run_dopri_process failed with code {rc}")
    for i, n in enumerate(emu._AD_F[:4]):
        adaptive[n][:] = fs[i]
    for i, n in enumerate(emu._AD_I[:4]):
        adaptive[n][:] = isv[i]
    return int(counters[0]), int(counters[1])
