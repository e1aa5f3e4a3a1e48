"""Observation / action wrappers of the gym_jiminy pipeline for the vectorised, device-resident environments
(reference python/gym_jiminy/common/gym_jiminy/common/wrappers/: observation_stack.py, normalize.py,
flatten.py).  They wrap anything with the `reset / step / observation` surface of `VecJiminyEnv`; observations are
nested dicts of tensors with a leading batch axis, and stay on the device.

* `StackObservation(env, num_stack, nested_filter_keys, skip_frames_ratio)`: rolling stack of the selected leaves;
  a stacked leaf `(B, ...)` becomes `(B, num_stack, ...)`, oldest first, the latest frame always the current value
  (observation_stack.py:40-265).  Lanes that were re-initialised restart with a zero history.
* `NormalizeObservation(env, bounds)` / `NormalizeAction(env, low, high)`: affine map of bounded leaves to [-1, 1]
  from pre-defined bounds, without clipping (normalize.py:49-114); unbounded leaves are left as they are
  (`ignore_unbounded`).
* `FlattenObservation(env)`: all leaves concatenated into one `(B, D)` tensor, keys in sorted order (flatten.py).
* `AdaptLayoutObservation(env, layout)` / `FilterObservation(env, nested_filter_keys)`: subtrees, leaves and blocks of leaves
  re-arranged into another nested structure, as views (observation_layout.py:36-311, :314-443, :446-540).  A block spec addresses
  the dimensions of a leaf behind its batch axis.
* `ScaleObservation(env, nested_scale)` / `ScaleAction(env, nested_scale)`: scalar factors on subtrees, leaves or blocks of leaves;
  the observation side divides (one rounded multiplication by `1.0 / scale` per operation), the action side multiplies
  (scale.py:31-84, :141-244, :247-end).  The action of these environments is one `(B, M)` tensor, so `FlattenAction` would be
  the identity and does not exist here.
* `AssembleObservation(env, ...)`: the chain `FlattenObservation(StackObservation(NormalizeObservation(ScaleObservation(
  AdaptLayoutObservation(env)))))` as ONE kernel launch per step (`blocks.ObservationAssembler`, csrc/jm_observe.h).
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

Path = Tuple[Union[str, int], ...]


def flatten_with_path(tree: Any, prefix: Path = ()) -> List[Tuple[Path, torch.Tensor]]:
    """Leaves of a nested dict / list / tuple of tensors with their paths, dict keys in sorted order."""
    if isinstance(tree, dict):
        out: List[Tuple[Path, torch.Tensor]] = []
        for k in sorted(tree):
            out += flatten_with_path(tree[k], prefix + (k,))
        return out
    if isinstance(tree, (list, tuple)):
        out = []
        for i, v in enumerate(tree):
            out += flatten_with_path(v, prefix + (i,))
        return out
    return [(prefix, tree)]


def _set_path(tree: Any, path: Path, value: Any) -> Any:
    """Copy-on-write update of one leaf of a nested dict / list / tuple."""
    if not path:
        return value
    if isinstance(tree, (list, tuple)):
        return type(tree)(_set_path(v, path[1:], value) if i == path[0] else v for i, v in enumerate(tree))
    new = dict(tree)
    new[path[0]] = _set_path(tree[path[0]], path[1:], value)
    return new


class _Wrapper:
    def __init__(self, env: Any) -> None:
        self.env = env

    def __getattr__(self, name: str) -> Any:   # everything else is the wrapped environment's
        return getattr(self.env, name)

    def transform(self, obs: Any) -> Any:
        return obs

    def observation(self) -> Any:
        """Current observation.  Read-only with respect to the wrapper's own state: wrappers that accumulate (the
        observation stack) update in `reset` / `step` only and answer here from what they hold (`peek`)."""
        return self.peek(self.env.observation())

    def peek(self, obs: Any) -> Any:
        return self.transform(obs)

    def reset(self, *args: Any, **kw: Any):
        obs, info = self.env.reset(*args, **kw)
        self._on_reset(None)
        return self.transform(obs), info

    def step(self, action: torch.Tensor):
        obs, reward, terminated, truncated, info = self.env.step(self.transform_action(action))
        if "reset_mask" in info:
            self._on_reset(info["reset_mask"])
        return self.transform(obs), reward, terminated, truncated, info

    def transform_action(self, action: torch.Tensor) -> torch.Tensor:
        return action

    def _on_reset(self, lane_mask: Optional[torch.Tensor]) -> None:
        pass


class StackObservation(_Wrapper):
    def __init__(self, env: Any, *, num_stack: int, nested_filter_keys: Optional[Sequence[Union[Path, str]]] = None,
                 skip_frames_ratio: int = -1) -> None:
        super().__init__(env)
        if num_stack < 1:
            raise ValueError("num_stack must be at least 1")
        self.num_stack = int(num_stack)
        # -1: one update per environment step (the only refresh granularity of the vectorised environments);
        # n >= 0: n steps skipped between two shifts of the stack
        self.skip_frames_ratio = int(skip_frames_ratio)
        keys = [(k,) if isinstance(k, (str, int)) else tuple(k) for k in (nested_filter_keys or [()])]
        self.nested_filter_keys: List[Path] = keys
        self._stack: Dict[Path, torch.Tensor] = {}
        self._n_since_shift = 0

    def _selected(self, path: Path) -> bool:
        return any(path[:len(k)] == k for k in self.nested_filter_keys)

    def _on_reset(self, lane_mask: Optional[torch.Tensor]) -> None:
        if lane_mask is None:
            self._stack.clear()
            self._n_since_shift = 0
            return
        for t in self._stack.values():
            m = lane_mask.view(-1, *([1] * (t.dim() - 1)))
            t.copy_(torch.where(m, torch.zeros_like(t), t))

    def transform(self, obs: Any) -> Any:
        leaves = [(p, x) for p, x in flatten_with_path(obs) if self._selected(p)]
        if not leaves:
            raise ValueError("At least one observation leaf must be stacked.")
        shift = self.skip_frames_ratio < 0 or self._n_since_shift >= self.skip_frames_ratio
        out = obs
        for path, x in leaves:
            st = self._stack.get(path)
            if st is None:
                st = torch.zeros((x.shape[0], self.num_stack) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
                self._stack[path] = st
            elif shift and self.num_stack > 1:
                st[:, :-1] = st[:, 1:].clone()
            st[:, -1] = x
            # (a copy: the ring buffer is rewritten by the next step, a rollout buffer that keeps the returned
            # observation must not see that)
            out = _set_path(out, path, st.clone())
        self._n_since_shift = 0 if shift else self._n_since_shift + 1
        return out

    def peek(self, obs: Any) -> Any:
        """The stack as it stands (copies), without shifting it: `observation()` between two steps."""
        out = obs
        for path, x in flatten_with_path(obs):
            if self._selected(path):
                st = self._stack.get(path)
                if st is None:   # nothing stacked yet: zeros and the current frame, like the first `transform`
                    st = torch.zeros((x.shape[0], self.num_stack) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
                    st[:, -1] = x
                out = _set_path(out, path, st.clone())
        return out


class NormalizeObservation(_Wrapper):
    def __init__(self, env: Any, bounds: Dict[Path, Tuple[Any, Any]], ignore_unbounded: bool = True) -> None:
        """`bounds`: `{path: (low, high)}` per leaf (broadcastable to the leaf without its batch axis)."""
        super().__init__(env)
        self.ignore_unbounded = ignore_unbounded
        self._bounds = {((p,) if isinstance(p, (str, int)) else tuple(p)): b for p, b in bounds.items()}
        self._maps: Dict[Path, Tuple[torch.Tensor, torch.Tensor]] = {}

    def _map(self, path: Path, x: torch.Tensor) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        if path in self._maps:
            return self._maps[path]
        if path not in self._bounds:
            if self.ignore_unbounded:
                return None
            raise ValueError(f"no bounds for observation leaf {path}")
        lo = torch.as_tensor(self._bounds[path][0], dtype=x.dtype, device=x.device).expand(x.shape[1:]).clone()
        hi = torch.as_tensor(self._bounds[path][1], dtype=x.dtype, device=x.device).expand(x.shape[1:]).clone()
        bounded = torch.isfinite(lo) & torch.isfinite(hi)
        if not bool(bounded.all()) and not self.ignore_unbounded:
            raise ValueError(f"observation leaf {path} is not bounded")
        # (x - mean) / scale with mean = (hi + lo) / 2, scale = (hi - lo) / 2; identity where unbounded
        mean = torch.where(bounded, 0.5 * (hi + lo), torch.zeros_like(lo))
        scale = torch.where(bounded, 0.5 * (hi - lo), torch.ones_like(lo))
        self._maps[path] = (mean, scale)
        return self._maps[path]

    def transform(self, obs: Any) -> Any:
        out = obs
        for path, x in flatten_with_path(obs):
            m = self._map(path, x)
            if m is not None:
                out = _set_path(out, path, (x - m[0]) / m[1])
        return out


class NormalizeAction(_Wrapper):
    def __init__(self, env: Any, low: Any, high: Any) -> None:
        """The policy acts in [-1, 1]^M; the environment receives `mean + scale * action` (no clipping)."""
        super().__init__(env)
        self._low, self._high = low, high
        self._map: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def transform_action(self, action: torch.Tensor) -> torch.Tensor:
        if self._map is None:
            lo = torch.as_tensor(self._low, dtype=action.dtype, device=action.device).expand(action.shape[1:])
            hi = torch.as_tensor(self._high, dtype=action.dtype, device=action.device).expand(action.shape[1:])
            bounded = torch.isfinite(lo) & torch.isfinite(hi)
            self._map = (torch.where(bounded, 0.5 * (hi + lo), torch.zeros_like(lo)),
                         torch.where(bounded, 0.5 * (hi - lo), torch.ones_like(lo)))
        return self._map[0] + self._map[1] * action


class FlattenObservation(_Wrapper):
    def __init__(self, env: Any, dtype: Optional[torch.dtype] = None, exclude: Iterable[Path] = (("t",),)) -> None:
        super().__init__(env)
        self._dtype = dtype
        self._exclude = [tuple(e) for e in exclude]

    def transform(self, obs: Any) -> torch.Tensor:
        parts = [x.reshape(x.shape[0], -1) for p, x in flatten_with_path(obs)
                 if not any(p[:len(e)] == e for e in self._exclude)]
        flat = torch.cat(parts, dim=1)
        return flat.to(self._dtype) if self._dtype is not None else flat


# ---------------------------------------------------------------------------------------------------- layout and scale
def _leaves_in_order(tree: Any, prefix: Path = ()) -> List[Tuple[Path, Any]]:
    """Leaves with their paths in the order of the containers themselves (the reference's `flatten_with_path` does not sort)."""
    if isinstance(tree, dict):
        return [leaf for k, v in tree.items() for leaf in _leaves_in_order(v, prefix + (k,))]
    if isinstance(tree, (list, tuple)):
        return [leaf for i, v in enumerate(tree) for leaf in _leaves_in_order(v, prefix + (i,))]
    return [(prefix, tree)]


def _as_path(key: Any) -> Path:
    return (key,) if isinstance(key, (str, int)) else tuple(key)


def _block_slices(block_spec: Sequence[Any]) -> Tuple[Any, ...]:
    """An array block spec -- per dimension an `int`, `()` or `(start, end)` -- as indices."""
    return tuple(b if isinstance(b, int) else (slice(None) if not b else slice(*b)) for b in block_spec)


def split_block_spec(nested_spec: Sequence[Any]) -> Tuple[Path, Optional[Tuple[Any, ...]]]:
    """`(nested key, indices of the block or None)` of a nested key that may end with an array block spec."""
    if nested_spec and isinstance(nested_spec[-1], (tuple, list)):
        return tuple(nested_spec[:-1]), _block_slices(nested_spec[-1])
    return tuple(nested_spec), None


class _Seq:
    """A sequence node of the layout under construction, with the type it ends as."""

    def __init__(self, items: Iterable[Any], kind: type) -> None:
        self.items, self.kind = list(items), kind


def _thaw(tree: Any) -> Any:
    if isinstance(tree, dict):
        return {k: _thaw(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return _Seq((_thaw(v) for v in tree), type(tree))
    return tree


def _freeze(tree: Any) -> Any:
    if isinstance(tree, dict):
        return {k: _freeze(v) for k, v in tree.items()}
    if isinstance(tree, _Seq):
        return tree.kind(_freeze(v) for v in tree.items)
    return tree


def _child(node: Any, key: Any) -> Any:
    return node.items[key] if isinstance(node, _Seq) else node[key]


def adapt_layout(data: Any, layout: Sequence[Tuple[Path, Sequence[Any]]], batch_axes: int = 1) -> Any:
    """≙ `_adapt_layout` (observation_layout.py:49-311) on nested dicts / lists / tuples of arrays: the entries
    `(nested_key_out, nested_spec_in)` are processed in order; a repeated output key aggregates into a tuple (or is appended
    to the sequence that is there already), an empty output key promotes the value.  Leaves are views; every container is
    new.  A block spec addresses the dimensions behind the first `batch_axes` ones."""
    out: Any = None
    for key_out, spec_in in layout:
        key_out = _as_path(key_out)
        if not spec_in:
            raise ValueError("Input nested keys must not be empty.")
        key_in, block = split_block_spec(spec_in)
        value = data
        try:
            for k in key_in:
                value = value[k]
        except (KeyError, IndexError, TypeError) as e:
            raise KeyError(f"Nested key '{key_in}' is missing.") from e
        if block is not None:
            value = value[(slice(None),) * batch_axes + block]
        value = _thaw(value)
        if not key_out:
            if out is None:
                out = value
            else:
                if not isinstance(out, _Seq):
                    out = _Seq([out], tuple)
                out.items.append(value)
            continue
        node = out
        for i, key in enumerate(key_out):
            last = i + 1 == len(key_out)
            if isinstance(key, str):
                if out is None:
                    node = out = {}
                if key not in node:
                    node[key] = value if last else {}
                    node = node[key]
                    continue
            elif out is None:
                node = out = _Seq([], tuple)
            if not last:
                node = _child(node, key)
                continue
            # the key is taken: what is there becomes (or is) a sequence and the value is appended
            there = _child(node, key)
            if not isinstance(there, _Seq):
                there = _Seq([there], tuple)
                if isinstance(node, _Seq):
                    node.items[key] = there
                else:
                    node[key] = there
            there.items.append(value)
    if out is None:
        raise ValueError("The resulting observation space must not be empty.")
    return _freeze(out)


class AdaptLayoutObservation(_Wrapper):
    def __init__(self, env: Any, layout: Sequence[Tuple[Any, Sequence[Any]]]) -> None:
        """≙ `AdaptLayoutObservation` (observation_layout.py:314-443)."""
        if not layout:
            raise ValueError("The resulting observation space must not be empty.")
        super().__init__(env)
        self.layout = [(_as_path(key_out), spec_in) for key_out, spec_in in layout]

    def transform(self, obs: Any) -> Any:
        return adapt_layout(obs, self.layout)


def filter_layout(obs: Any, nested_filter_keys: Sequence[Any]) -> List[Tuple[Path, Path]]:
    """The layout `FilterObservation` keeps (observation_layout.py:502-530): the leaves under the keys in their original
    order, each once; a leaf of a sequence is aggregated under the key of the sequence."""
    keys = [_as_path(k) for k in nested_filter_keys]
    kept: List[Path] = []
    for path, _ in _leaves_in_order(obs):
        if any(path[:len(k)] == k for k in keys) and path not in kept:
            kept.append(path)
    if not kept:
        raise ValueError("At least one observation leaf must be preserved.")
    return [(path[:-1] if isinstance(path[-1], int) else path, path) for path in kept]


class FilterObservation(_Wrapper):
    def __init__(self, env: Any, nested_filter_keys: Sequence[Any]) -> None:
        """≙ `FilterObservation` (observation_layout.py:446-540)."""
        super().__init__(env)
        if isinstance(nested_filter_keys, str):
            raise TypeError("nested_filter_keys is a sequence of nested keys")
        self.nested_filter_keys = [_as_path(k) for k in nested_filter_keys]
        self._layout: Optional[List[Tuple[Path, Path]]] = None

    def transform(self, obs: Any) -> Any:
        if self._layout is None:
            self._layout = filter_layout(obs, self.nested_filter_keys)
        return adapt_layout(obs, self._layout)


def _check_scale_keys(paths: Sequence[Path], nested_scale: Sequence[Tuple[Sequence[Any], float]], what: str
                      ) -> List[Tuple[Path, Optional[Tuple[Any, ...]], float]]:
    specs = []
    for nested_spec, scale in nested_scale:
        key, block = split_block_spec(nested_spec)
        key = tuple(k for k in key if k != ())        # (`((), block spec)`: the one tensor of these environments' action)
        if not any(path[:len(key)] == key for path in paths):
            raise ValueError(f"Nested key {key} not found in base {what} space.")
        if float(scale) == 0.0:
            raise ValueError(f"the scale of nested key {key} must not be zero")
        specs.append((key, block, float(scale)))
    return specs


def observation_scale_ops(paths: Sequence[Path], nested_scale: Sequence[Tuple[Sequence[Any], float]]
                          ) -> Dict[Path, List[Tuple[Optional[Tuple[Any, ...]], float]]]:
    """The operations `ScaleObservation` applies to every leaf, `(block or None, factor)` in order (scale.py:189-225): the
    full-leaf factors of a leaf are merged into one operation (`1.0 / (scale / previous factor)`), which comes first; the block
    operations follow in the order given, each with the factor `1.0 / scale`."""
    specs = _check_scale_keys(paths, nested_scale, "observation")
    ops: Dict[Path, List[Tuple[Optional[Tuple[Any, ...]], float]]] = {}
    for path in paths:
        full: Optional[float] = None
        blocks: List[Tuple[Optional[Tuple[Any, ...]], float]] = []
        for key, block, scale in specs:
            if path[:len(key)] != key:
                continue
            if block is None:
                if full is not None:
                    scale = scale / full
                full = 1.0 / scale
            else:
                blocks.append((block, 1.0 / scale))
        if full is not None or blocks:
            ops[path] = ([(None, full)] if full is not None else []) + blocks
    return ops


class ScaleObservation(_Wrapper):
    def __init__(self, env: Any, nested_scale: Sequence[Tuple[Sequence[Any], float]]) -> None:
        """≙ `ScaleObservation` (scale.py:141-244): `nested_scale` is a sequence of `(nested key, possibly ending with an array
        block spec; scale)`.  Unknown keys are refused at the first observation."""
        super().__init__(env)
        self.nested_scale = list(nested_scale)
        self._ops: Optional[Dict[Path, List[Tuple[Optional[Tuple[Any, ...]], float]]]] = None

    def transform(self, obs: Any) -> Any:
        leaves = flatten_with_path(obs)
        if self._ops is None:
            self._ops = observation_scale_ops([p for p, _ in leaves], self.nested_scale)
        out = obs
        for path, x in leaves:
            ops = self._ops.get(path)
            if not ops:
                continue
            if ops[0][0] is None:
                y = x * ops[0][1]
                ops = ops[1:]
            else:
                y = x.clone()
            for block, factor in ops:
                view = y[(slice(None),) + block]
                view.mul_(factor)
            out = _set_path(out, path, y)
        return out


def action_scale_ops(nested_scale: Sequence[Tuple[Sequence[Any], float]]) -> List[Tuple[Optional[Tuple[Any, ...]], float]]:
    """The operations `ScaleAction` applies to the action tensor, `(block or None, factor)` in order (scale.py:292-305): the
    factors given for one and the same block are multiplied into one operation at the place of the first; the full-tensor
    operation comes first."""
    ops: Dict[Any, Tuple[Optional[Tuple[Any, ...]], float]] = {}
    for key, block, scale in _check_scale_keys([()], nested_scale, "action"):
        name = None if block is None else repr(block)       # (a `slice` is not hashable before Python 3.12)
        ops[name] = (block, scale * ops[name][1] if name in ops else scale * 1.0)
    return ([ops[None]] if None in ops else []) + [op for name, op in ops.items() if name is not None]


class ScaleAction(_Wrapper):
    def __init__(self, env: Any, nested_scale: Sequence[Tuple[Sequence[Any], float]]) -> None:
        """≙ `ScaleAction` (scale.py:247-end): the environment receives the action multiplied by the factors.  The action is
        one `(B, M)` tensor: a key is `()` or `((), block spec)`."""
        super().__init__(env)
        self.nested_scale = list(nested_scale)
        self._ops = action_scale_ops(self.nested_scale)

    def transform_action(self, action: torch.Tensor) -> torch.Tensor:
        ops = self._ops
        if ops and ops[0][0] is None:
            out = action * ops[0][1]
            ops = ops[1:]
        else:
            out = action.clone()
        for block, factor in ops:
            view = out[(slice(None),) + block]
            view.mul_(factor)
        return out


# -------------------------------------------------------------------------------------------------- the assembled chain
class AssembleObservation(_Wrapper):
    """`FlattenObservation(StackObservation(NormalizeObservation(ScaleObservation(AdaptLayoutObservation(env)))))` as one
    kernel launch per step: `reset`, `step` and `observation()` return the `(B, W)` tensor of `dtype` that the chain of
    tensor wrappers with the same arguments returns, bit for bit.  A stage whose argument is None (`num_stack` 1 for the
    stack) is left out.  `nested_scale`, `bounds` and `nested_filter_keys` address the observation behind the layout.

    The returned tensor is the assembler's own and is rewritten by the next step: a rollout buffer copies it (`Tensor.copy_`
    into its storage), which the tensor wrappers do on every step for every stacked leaf.  `step` adds one launch to the
    environment's and no tensor operation.  With JIMINY_AMD_TENSOR_BLOCKS=1 the chain of tensor wrappers runs instead."""

    def __init__(self, env: Any, *, layout: Optional[Sequence[Tuple[Any, Sequence[Any]]]] = None,
                 nested_scale: Optional[Sequence[Tuple[Sequence[Any], float]]] = None,
                 bounds: Optional[Dict[Path, Tuple[Any, Any]]] = None, ignore_unbounded: bool = True, num_stack: int = 1,
                 nested_filter_keys: Optional[Sequence[Union[Path, str]]] = None, skip_frames_ratio: int = -1,
                 dtype: Optional[torch.dtype] = torch.float32, exclude: Iterable[Path] = (("t",),)) -> None:
        import os
        super().__init__(env)
        if num_stack < 1:
            raise ValueError("num_stack must be at least 1")
        if layout is not None and not layout:
            raise ValueError("The resulting observation space must not be empty.")
        self.num_stack, self.skip_frames_ratio = int(num_stack), int(skip_frames_ratio)
        self._spec = dict(layout=layout, nested_scale=nested_scale, bounds=bounds, ignore_unbounded=ignore_unbounded,
                          num_stack=self.num_stack, nested_filter_keys=nested_filter_keys, dtype=dtype,
                          exclude=tuple(tuple(e) for e in exclude))
        self._n_since_shift = 0
        self._chain: Any = None
        self._assembler: Any = None
        if os.environ.get("JIMINY_AMD_TENSOR_BLOCKS", "0") == "1":
            self._chain = self._tensor_chain(env)

    def _tensor_chain(self, env: Any) -> Any:
        spec, chain = self._spec, env
        if spec["layout"] is not None:
            chain = AdaptLayoutObservation(chain, spec["layout"])
        if spec["nested_scale"] is not None:
            chain = ScaleObservation(chain, spec["nested_scale"])
        if spec["bounds"] is not None:
            chain = NormalizeObservation(chain, spec["bounds"], spec["ignore_unbounded"])
        if self.num_stack > 1:
            chain = StackObservation(chain, num_stack=self.num_stack, nested_filter_keys=spec["nested_filter_keys"],
                                     skip_frames_ratio=self.skip_frames_ratio)
        return FlattenObservation(chain, dtype=spec["dtype"], exclude=spec["exclude"])

    def _assemble(self, obs: Any, shift: bool, reset_mask: Optional[torch.Tensor]) -> torch.Tensor:
        if self._assembler is None:
            from .blocks import ObservationAssembler
            self._assembler = ObservationAssembler(self._engine_of(self.env), obs, **self._spec)
        self._assembler.refresh(shift=shift, reset_mask=reset_mask, obs=obs)
        return self._assembler.out

    @staticmethod
    def _engine_of(env: Any) -> Any:
        while True:
            engine = getattr(env, "engine", None)
            if engine is not None:
                return engine
            if not hasattr(env, "env"):
                raise ValueError("AssembleObservation wraps an environment that has an `engine`")
            env = env.env

    def _next_shift(self) -> bool:
        # (the counter of `StackObservation.transform`)
        shift = self.skip_frames_ratio < 0 or self._n_since_shift >= self.skip_frames_ratio
        self._n_since_shift = 0 if shift else self._n_since_shift + 1
        return shift

    def reset(self, *args: Any, **kw: Any):
        if self._chain is not None:
            return self._chain.reset(*args, **kw)
        obs, info = self.env.reset(*args, **kw)
        self._n_since_shift = 0
        if self._assembler is not None:
            self._assembler.reset()
        self._next_shift()      # (the first frame of an empty stack is written, not shifted in)
        return self._assemble(obs, False, None), info

    def step(self, action: torch.Tensor):
        if self._chain is not None:
            return self._chain.step(action)
        obs, reward, terminated, truncated, info = self.env.step(self.transform_action(action))
        return self._assemble(obs, self._next_shift(), info.get("reset_mask")), reward, terminated, truncated, info

    def observation(self) -> torch.Tensor:
        if self._chain is not None:
            return self._chain.observation()
        return self.peek(self.env.observation())

    def peek(self, obs: Any) -> torch.Tensor:
        """The assembled observation as it stands; before the first `reset` or `step`: zeros and the current frame."""
        if self._chain is not None:
            return self._chain.peek(obs)
        if self._assembler is None:
            return self._assemble(obs, False, None)
        return self._assembler.out

    def transform(self, obs: Any) -> torch.Tensor:
        if self._chain is not None:
            return self._chain.transform(obs)
        return self._assemble(obs, self._next_shift(), None)
