"""Build + ctypes driver of the jm_math.h probe (tests/device_math/jm_math_probe.hip): the gfx950 library, built with the
kernels' flags (jiminy_amd.codegen.build_probe), and its host twin, built with the host emulation's compiler and flags
(tests.hostemu.emu.host_compiler, -DJM_HOST_EMU)."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from jiminy_amd import codegen

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(_HERE))
SRC = os.path.join(_HERE, "jm_math_probe.hip")
OUT_DIR = os.path.join(ROOT, "build", "device_math")
DEVICE_LIB = os.path.join(OUT_DIR, "libjm_math_probe.so")
HOST_LIB = os.path.join(OUT_DIR, "libjm_math_probe_host.so")

# order and arity of `enum Op` in the probe source
OPS = ("sincos", "tanh", "rcp", "rsqrt", "sqrt", "exp6", "log3", "matrix_to_quat", "quat_to_matrix", "quat_exp3",
       "quat_log3", "quat_mul", "jlog3_mul", "sym_inverse", "rot_rodrigues")
NIN = dict(zip(OPS, (1, 1, 1, 1, 1, 6, 9, 9, 4, 3, 4, 8, 7, 6, 5)))
NOUT = dict(zip(OPS, (2, 1, 1, 1, 1, 12, 3, 4, 9, 4, 4, 4, 3, 6, 9)))
MODES = {"all": 0, "divergent": 1, "ragged": 2}
SENTINEL = {np.float64: np.uint64(0x7FF4DEADBEEF0001), np.float32: np.uint32(0x7FA0BEEF)}   # signalling NaNs with a payload

_LIBS = {}


def build_device(force: bool = False) -> str:
    return codegen.build_probe(SRC, DEVICE_LIB, force=force)


def build_host(force: bool = False) -> str:
    from tests.hostemu.emu import host_compiler
    cmd = host_compiler() + ["-DJM_HOST_EMU", "-x", "c++", SRC, "-o", HOST_LIB + ".tmp"]
    h = hashlib.sha256(" ".join(cmd).encode())
    for path in (SRC, os.path.join(codegen.CSRC, "jm_math.h")):
        with open(path, "rb") as f:
            h.update(f.read())
    try:
        with open(HOST_LIB + ".src") as f:
            fresh = f.read().strip() == h.hexdigest() and os.path.exists(HOST_LIB)
    except OSError:
        fresh = False
    if force or not fresh:
        os.makedirs(OUT_DIR, exist_ok=True)
        subprocess.check_call(cmd)
        os.replace(HOST_LIB + ".tmp", HOST_LIB)
        with open(HOST_LIB + ".src", "w") as f:
            f.write(h.hexdigest() + "\n")
    return HOST_LIB


def _load(path: str) -> C.CDLL:
    if path not in _LIBS:
        L = C.CDLL(path)
        for name in ("jm_probe_f64", "jm_probe_f32"):
            getattr(L, name).argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            getattr(L, name).restype = C.c_int
        _LIBS[path] = L
    return _LIBS[path]


def _prepare(op: str, x: np.ndarray, dtype):
    x = np.ascontiguousarray(np.asarray(x, dtype=dtype).reshape(-1, NIN[op]))
    out = np.full((x.shape[0], NOUT[op]), SENTINEL[dtype]).view(dtype)
    return x, out


def host(op: str, x: np.ndarray, dtype=np.float64, mode: str = "all") -> np.ndarray:
    """The host twin applied to the rows of `x`; rows a mode skips keep the sentinel."""
    L = _load(build_host())
    x, out = _prepare(op, x, dtype)
    fn = L.jm_probe_f64 if dtype == np.float64 else L.jm_probe_f32
    rc = fn(OPS.index(op), x.ctypes.data, out.ctypes.data, x.shape[0], MODES[mode])
    if rc != 0:
        raise RuntimeError(f"host probe {op} failed ({rc})")
    return out


def device(op: str, x: np.ndarray, dtype=np.float64, mode: str = "all") -> np.ndarray:
    """The gfx950 build applied to the rows of `x` on cuda:0.  The library is built by __graft_entry__.build()."""
    import torch
    if not os.path.exists(DEVICE_LIB):
        raise RuntimeError(f"{DEVICE_LIB} is missing: run `python __graft_entry__.py` (build()) first")
    L = _load(DEVICE_LIB)
    x, out = _prepare(op, x, dtype)
    dx = torch.from_numpy(x).cuda()
    dout = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    fn = L.jm_probe_f64 if dtype == np.float64 else L.jm_probe_f32
    rc = fn(OPS.index(op), dx.data_ptr(), dout.data_ptr(), x.shape[0], MODES[mode])
    if rc != 0:
        raise RuntimeError(f"device probe {op} failed ({rc})")
    return dout.cpu().numpy()
