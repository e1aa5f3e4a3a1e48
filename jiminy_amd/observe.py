"""From a nested observation of device tensors and the arguments of the observation wrappers to the plan that
`jm_block_observe` interprets on the device (csrc/jm_observe.h): what
`FlattenObservation(StackObservation(NormalizeObservation(ScaleObservation(AdaptLayoutObservation(env)))))` computes, stated per
*element* (one scalar of one kept leaf: source slot and row, multipliers, mean and scale) and per *position* (one column of the
output: element and age).

A leaf is a batch-first view of `[rows...][B]` storage in the engine dtype -- `leaf.movedim(0, -1)` is contiguous -- which is what
`VecJiminyEnv.observation()` and `PDControlledWalkerVecEnv.observation()` return; anything else is refused with its path.  The
layout is applied to arrays of row indices with the very function the tensor wrapper uses (`wrappers.adapt_layout`), the scale
operations are those of `wrappers.observation_scale_ops`, the normalisation constants are computed in the engine dtype as
`NormalizeObservation` does, and the flat order is that of `FlattenObservation` over the stacked leaves.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _abi
from .wrappers import Path, _as_path, adapt_layout, flatten_with_path, observation_scale_ops

# caps of csrc/jm_observe.h
MAX_SOURCES, MAX_ELEMENTS, MAX_STACK, MAX_POSITIONS, MAX_MULTIPLIERS = 16, 2048, 16, 8192, 4
_ROW_BITS = 32


@dataclass
class ObservePlan:
    arrays: Dict[str, Any]              # the fields of `jm_observe_desc`
    source_paths: List[Path]            # the leaf of the environment's observation behind every slot
    leaf_paths: List[Path]              # the kept leaves of the assembled observation, in flat order
    leaf_stacked: List[bool]
    dtype_in: torch.dtype
    dtype_out: torch.dtype

    @property
    def n_elements(self) -> int:
        return len(self.arrays["elem_slot"])

    @property
    def n_positions(self) -> int:
        return len(self.arrays["pos_elem"])

    @property
    def num_stack(self) -> int:
        return int(self.arrays["num_stack"])

    def desc(self) -> Tuple["_abi.ObserveDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(**arrays) -> Tuple["_abi.ObserveDesc", List[np.ndarray]]:
    """`jm_observe_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    import ctypes as C
    d = _abi.ObserveDesc()
    keep: List[np.ndarray] = []
    for name in _abi.OBSERVE_DESC_INTS:
        a = _abi._i32(arrays[name])
        keep.append(a)
        setattr(d, name, a.ctypes.data_as(C.POINTER(C.c_int32)))
    for name in _abi.OBSERVE_DESC_DOUBLES:
        a = _abi._f64(arrays[name])
        keep.append(a)
        setattr(d, name, a.ctypes.data_as(C.POINTER(C.c_double)))
    d.n_sources = len(arrays["source_rows"])
    d.n_elements = len(arrays["elem_slot"])
    d.n_multipliers = len(arrays["multiplier"])
    d.num_stack = int(arrays["num_stack"])
    d.n_positions = len(arrays["pos_elem"])
    return d, keep


def check_dtypes(dtype_in: torch.dtype, dtype_out: torch.dtype) -> None:
    if dtype_in not in (torch.float64, torch.float32) or dtype_out not in (torch.float64, torch.float32):
        raise ValueError("the observation assembly works on float64 and float32")
    if dtype_in == torch.float32 and dtype_out == torch.float64:
        raise ValueError("float32 sources with a float64 output are not supported (float64 -> float64, float64 -> float32, "
                         "float32 -> float32)")


def is_lane_minor(leaf: torch.Tensor) -> bool:
    """The leaf is a batch-first view of `[rows...][B]` storage."""
    return leaf.dim() >= 1 and leaf.movedim(0, -1).is_contiguous()


def _map_leaves(fn, tree: Any, prefix: Path = ()) -> Any:
    if isinstance(tree, dict):
        return {k: _map_leaves(fn, v, prefix + (k,)) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_map_leaves(fn, v, prefix + (i,)) for i, v in enumerate(tree))
    return fn(prefix, tree)


def normalization_constants(bounds: Tuple[Any, Any], shape: Tuple[int, ...], dtype: torch.dtype, path: Path,
                            ignore_unbounded: bool) -> Tuple[np.ndarray, np.ndarray]:
    """`mean`, `scale` of `NormalizeObservation._map`, computed in `dtype` on the host (IEEE basic operations: the device
    gives the same bits) and widened to float64, which is exact."""
    lo = torch.as_tensor(bounds[0], dtype=dtype).expand(shape).clone()
    hi = torch.as_tensor(bounds[1], dtype=dtype).expand(shape).clone()
    bounded = torch.isfinite(lo) & torch.isfinite(hi)
    if not bool(bounded.all()) and not ignore_unbounded:
        raise ValueError(f"observation leaf {path} is not bounded")
    mean = torch.where(bounded, 0.5 * (hi + lo), torch.zeros_like(lo))
    scale = torch.where(bounded, 0.5 * (hi - lo), torch.ones_like(lo))
    if bool((scale == 0).any()):
        raise ValueError(f"observation leaf {path} has a zero scale: its bounds coincide")
    return mean.double().numpy().reshape(-1), scale.double().numpy().reshape(-1)


def build_plan(obs: Any, *, layout: Optional[Sequence[Tuple[Any, Sequence[Any]]]] = None,
               nested_scale: Optional[Sequence[Tuple[Sequence[Any], float]]] = None,
               bounds: Optional[Dict[Any, Tuple[Any, Any]]] = None, ignore_unbounded: bool = True, num_stack: int = 1,
               nested_filter_keys: Optional[Sequence[Union[Path, str]]] = None, dtype: Optional[torch.dtype] = torch.float32,
               exclude: Iterable[Path] = (("t",),), engine_dtype: Optional[torch.dtype] = None) -> ObservePlan:
    sources = flatten_with_path(obs)
    if engine_dtype is None:
        engine_dtype = next((x.dtype for _, x in sources if x.is_floating_point() and x.dim() > 1), torch.float64)
    dtype_out = engine_dtype if dtype is None else dtype
    check_dtypes(engine_dtype, dtype_out)
    num_stack = int(num_stack)
    if num_stack < 1:
        raise ValueError("num_stack must be at least 1")
    if num_stack > MAX_STACK:
        raise ValueError(f"num_stack must be in [1, {MAX_STACK}], got {num_stack}")
    if layout is not None and not layout:
        raise ValueError("The resulting observation space must not be empty.")
    # every leaf as the array of its rows, tagged with the leaf; the layout moves those exactly as it moves the tensors
    ids = {path: i for i, (path, _) in enumerate(sources)}
    index_tree = _map_leaves(lambda path, x: (np.arange(int(np.prod(x.shape[1:], dtype=np.int64)), dtype=np.int64)
                                              + (ids[path] << _ROW_BITS)).reshape(tuple(x.shape[1:])), obs)
    if layout is not None:
        index_tree = adapt_layout(index_tree, [(_as_path(k), spec) for k, spec in layout], batch_axes=0)
    leaves = flatten_with_path(index_tree)
    paths = [p for p, _ in leaves]
    scale_ops = observation_scale_ops(paths, nested_scale) if nested_scale is not None else {}
    norm = {_as_path(p): b for p, b in (bounds or {}).items()}
    if bounds is not None and not ignore_unbounded:
        for p in paths:
            if p not in norm:
                raise ValueError(f"no bounds for observation leaf {p}")
    stack_keys = [_as_path(k) for k in (nested_filter_keys or [()])]
    if num_stack > 1 and not any(p[:len(k)] == k for p in paths for k in stack_keys):
        raise ValueError("At least one observation leaf must be stacked.")
    exclude = [tuple(e) for e in exclude]
    slot_of: Dict[int, int] = {}
    arrays: Dict[str, Any] = {k: [] for k in ("source_rows", "elem_slot", "elem_row", "elem_mult_start", "elem_mult_count",
                                              "elem_mean", "elem_scale", "multiplier", "pos_elem", "pos_age")}
    arrays["num_stack"] = num_stack
    source_paths: List[Path] = []
    leaf_paths: List[Path] = []
    leaf_stacked: List[bool] = []
    for path, index in leaves:
        if any(path[:len(e)] == e for e in exclude):
            continue
        index = np.asarray(index)
        flat = index.reshape(-1)
        n = flat.size
        if n == 0:
            continue
        for leaf_id in dict.fromkeys(int(i) for i in flat >> _ROW_BITS):
            if leaf_id in slot_of:
                continue
            src_path, x = sources[leaf_id]
            if x.dtype != engine_dtype or not is_lane_minor(x):
                raise ValueError(f"observation leaf {src_path} is not a batch-first view of [rows][B] storage in the engine dtype "
                                 f"({engine_dtype}): {x.dtype}, shape {tuple(x.shape)}, strides {tuple(x.stride())}")
            if len(slot_of) >= MAX_SOURCES:
                raise ValueError(f"1 to {MAX_SOURCES} sources are supported, got {len(slot_of) + 1}: leaf {src_path} is one too many")
            slot_of[leaf_id] = len(slot_of)
            source_paths.append(src_path)
            arrays["source_rows"].append(max(1, int(np.prod(x.shape[1:], dtype=np.int64))))
        chains: List[List[float]] = [[] for _ in range(n)]
        for block, factor in scale_ops.get(path, []):
            hit = np.zeros(index.shape, dtype=bool)
            hit[() if block is None else block] = True
            for j in np.flatnonzero(hit.reshape(-1)):
                chains[j].append(factor)
        if path in norm:
            mean, scale = normalization_constants(norm[path], tuple(index.shape), engine_dtype, path, ignore_unbounded)
        else:
            mean, scale = np.zeros(n), np.ones(n)
        e0 = len(arrays["elem_slot"])
        for j in range(n):
            if len(chains[j]) > MAX_MULTIPLIERS:
                raise ValueError(f"element {j} of observation leaf {path} has {len(chains[j])} multipliers, at most "
                                 f"{MAX_MULTIPLIERS} per element are supported")
            arrays["elem_slot"].append(slot_of[int(flat[j] >> _ROW_BITS)])
            arrays["elem_row"].append(int(flat[j] & ((1 << _ROW_BITS) - 1)))
            arrays["elem_mult_start"].append(len(arrays["multiplier"]))
            arrays["elem_mult_count"].append(len(chains[j]))
            arrays["multiplier"] += chains[j]
            arrays["elem_mean"].append(float(mean[j]))
            arrays["elem_scale"].append(float(scale[j]))
        stacked = num_stack > 1 and any(path[:len(k)] == k for k in stack_keys)
        for s in range(num_stack if stacked else 1):        # oldest first
            arrays["pos_elem"] += list(range(e0, e0 + n))
            arrays["pos_age"] += [(num_stack - 1 - s) if stacked else 0] * n
        leaf_paths.append(path)
        leaf_stacked.append(stacked)
    if not arrays["elem_slot"]:
        raise ValueError("The resulting observation space must not be empty.")
    if len(arrays["elem_slot"]) > MAX_ELEMENTS:
        raise ValueError(f"at most {MAX_ELEMENTS} elements are supported, got {len(arrays['elem_slot'])}")
    if len(arrays["pos_elem"]) > MAX_POSITIONS:
        raise ValueError(f"1 to {MAX_POSITIONS} output positions are supported, got {len(arrays['pos_elem'])}")
    return ObservePlan(arrays=arrays, source_paths=source_paths, leaf_paths=leaf_paths, leaf_stacked=leaf_stacked,
                       dtype_in=engine_dtype, dtype_out=dtype_out)


def source_tensors(obs: Any, plan: ObservePlan) -> List[torch.Tensor]:
    """The leaf behind every slot of the plan in a (new) observation of the same environment."""
    out = []
    for path in plan.source_paths:
        x = obs
        for k in path:
            x = x[k]
        out.append(x)
    return out


def check_no_alias(out: torch.Tensor, others: Sequence[Tuple[str, torch.Tensor]]) -> None:
    """`out` shares no byte with a source or the history (the check `jm_block_observe` repeats at every launch)."""
    def span(t: torch.Tensor) -> Tuple[int, int]:
        n = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) if t.numel() else 0
        return t.data_ptr(), t.data_ptr() + n * t.element_size()
    a0, a1 = span(out)
    for name, t in others:
        b0, b1 = span(t)
        if a0 < b1 and b0 < a1:
            raise ValueError(f"out aliases {name}")
