"""Host side of the composition layer: the reference's reward and termination classes as descriptions, and the plan
`jm_block_compose` interprets on the device (csrc/jm_compose.h).

Reference (python/gym_jiminy/common/gym_jiminy/common): `bases/compositions.py:88-663` (`AbstractReward`, `QuantityReward`,
`MixtureReward`, `QuantityTermination`), `compositions/mixin.py:108-258` (`AdditiveMixtureReward`,
`MultiplicativeMixtureReward`), `compositions/generic.py:32-61` (`SurviveReward`).  The classes here take the reference's
constructor arguments minus `env`; a leaf is not a quantity with a transform but a row `[B]` of a tensor a block left on the
device, a termination reads a view `[..., B]` of such a tensor.  The constructors derive `is_terminal` and `is_normalized` of a
mixture, drop the components whose weight is not positive, raise and warn as the reference's do.

Three behaviours of the reference that hold here as well: an indefinite component or mixture (`is_terminal=None`,
which a mixture of terminal and non-terminal components is) is evaluated like a non-terminal one and skipped at termination;
a termination on rows `[n][B]` fires on NaN, one on a single row `[B]` does not; the L^inf norm skips a NaN behind the first
component.  `order='inf'` is `float('inf')` here (the reference's string never reaches `weighted_norm` as a number).
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._plan import fill_desc

LOGGER = logging.getLogger(__name__)

# caps of csrc/jm_compose.h
MAX_SOURCES, MAX_NODES, MAX_DEPTH, MAX_CONDITIONS, MAX_ELEMENTS = 16, 32, 4, 16, 64
SRC_DTYPE, SRC_INT32, SRC_UINT8 = 0, 1, 2
LEAF, SURVIVE, ADDITIVE, MULTIPLICATIVE = 0, 1, 2, 3
COND_ARRAY, COND_TRUNCATION, COND_TRAINING_ONLY = 1, 2, 4
HAS_LOW, HAS_HIGH = 1, 2


class SurviveReward:
    """≙ `SurviveReward` (compositions/generic.py:32-61): 1.0 on every step but the terminal one, where it is not evaluated."""
    name, is_terminal, is_normalized = "reward_survive", False, True


class RewardTerm:
    """≙ `QuantityReward` without its transform: the value is the row `[B]` of a block tensor (a view; or, handed to
    `WalkerVecEnv(reward=...)`, None: the name is then one of the environment's reward rows).  `is_terminal`: True (evaluated on
    the terminal step only), False (on every other step) or None (indefinite: evaluated like False)."""

    def __init__(self, name: str, row: Any = None, *, is_normalized: bool = True, is_terminal: Optional[bool] = False) -> None:
        self.name, self.row, self.is_normalized, self.is_terminal = str(name), row, bool(is_normalized), is_terminal


def _component(c: Any):
    return RewardTerm(c) if isinstance(c, str) else c


class _Mixture:
    def __init__(self, name: str, components: Sequence[Any], is_normalized: bool) -> None:
        if not components:
            raise ValueError("At least one reward component must be specified.")        # (bases/compositions.py:374-376)
        self.name, self.components, self.is_normalized = str(name), tuple(components), bool(is_normalized)
        is_terminal = {c.is_terminal for c in self.components}                         # (:392-396)
        self.is_terminal = next(iter(is_terminal)) if len(is_terminal) == 1 else None


class AdditiveMixtureReward(_Mixture):
    """≙ `AdditiveMixtureReward` (compositions/mixin.py:108-190): the weighted L^p norm of the evaluated components, `order` any
    p > 0, `float('inf')` or 'inf'.  A component may be the name of a reward row of the environment."""

    def __init__(self, name: str, components: Sequence[Any], order: Union[int, float, str] = 1,
                 weights: Optional[Sequence[float]] = None) -> None:
        components = [_component(c) for c in components]
        if weights is None:
            weights = (1.0 / len(components),) * len(components)
        if isinstance(order, str):
            if order != "inf":
                raise ValueError("'order' must be strictly positive or 'inf'.")
            order = float("inf")
        if not order > 0.0:
            raise ValueError("'order' must be strictly positive or 'inf'.")
        if len(weights) != len(components):
            raise ValueError("Exactly one weight per reward component must be specified.")
        kept = [(float(w), c) for w, c in zip(weights, components) if w > 0.0]
        if not kept:
            raise ValueError("At least one reward component must have a positive weight.")
        scale, is_normalized = 0.0, True
        for weight, reward in kept:
            if not reward.is_normalized:
                LOGGER.warning("Reward '%s' is not normalized. Aggregating rewards that are not normalized using the addition "
                               "operator is not recommended.", reward.name)
                is_normalized = False
                break
            scale = max(scale, weight) if order == float("inf") else scale + weight
        else:
            is_normalized = abs(1.0 - scale) < 1e-4
        self.order, self.weights = float(order), tuple(w for w, _ in kept)
        super().__init__(name, [c for _, c in kept], is_normalized)


class MultiplicativeMixtureReward(_Mixture):
    """≙ `MultiplicativeMixtureReward` (compositions/mixin.py:225-249): the geometric mean of the evaluated components."""

    def __init__(self, name: str, components: Sequence[Any]) -> None:
        components = [_component(c) for c in components]
        super().__init__(name, components, all(c.is_normalized for c in components))


class Termination:
    """≙ `QuantityTermination` (bases/compositions.py:577-663): the episode ends where an element of `rows` leaves
    [`low`, `high`] (each None, a number, or one number per element).  `rows`: a view `[..., B]` of a block tensor; a single row
    `[B]` is the reference's 0-d quantity, which NaN does not fire, anything with more dimensions its array, which NaN fires.
    Handed to `WalkerVecEnv(termination_conditions=...)`, `rows` may be None: the name is then one of the environment's."""

    def __init__(self, name: str, rows: Any, low: Any, high: Any, grace_period: float = 0.0, *, is_truncation: bool = False,
                 training_only: bool = False) -> None:
        self.name, self.rows, self.low, self.high = str(name), rows, low, high
        self.grace_period, self.is_truncation, self.training_only = float(grace_period), bool(is_truncation), bool(training_only)


@dataclass
class ComposePlan:
    node_names: List[str]
    condition_names: List[str]
    arrays: Dict[str, Any] = field(default_factory=dict)
    sources: List[Any] = field(default_factory=list)        # the tensor that keeps slot s alive
    source_ptr: List[int] = field(default_factory=list)     # its base pointer

    @property
    def n_nodes(self) -> int:
        return len(self.node_names)

    def desc(self) -> Tuple["_abi.ComposeDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(**arrays) -> Tuple["_abi.ComposeDesc", List[np.ndarray]]:
    """`jm_compose_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.ComposeDesc()
    a, keep = fill_desc(d, {k: arrays[k] for k in _abi.COMPOSE_DESC_INTS}, {k: arrays[k] for k in _abi.COMPOSE_DESC_DOUBLES})
    d.n_sources, d.n_nodes, d.n_children = len(a["source_kind"]), len(a["node_kind"]), len(a["child"])
    d.n_conditions, d.n_elements = len(a["cond_flags"]), len(a["elem_slot"])
    return d, keep


class _Sources:
    """The slot table: one slot per storage a row lies in."""

    def __init__(self, batch_size: int, dtype) -> None:
        self.B, self.dtype = int(batch_size), dtype
        self.keys: List[Tuple[int, int]] = []
        self.tensors: List[Any] = []
        self.rows: List[int] = []

    def locate(self, t: Any, who: str) -> List[Tuple[int, int]]:
        """(slot, row) of every element of the view `t` `[..., B]`, in C order."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: expected a view of a block tensor, got {type(t).__name__}")
        kinds = {self.dtype: SRC_DTYPE, torch.int32: SRC_INT32, torch.uint8: SRC_UINT8, torch.bool: SRC_UINT8}
        if t.dtype not in kinds:
            raise ValueError(f"{who}: rows must be of the engine dtype, int32, uint8 or bool, got {t.dtype}")
        B = self.B
        if t.dim() < 1 or t.shape[-1] != B or (B > 1 and t.stride(-1) != 1):
            raise ValueError(f"{who}: expected a view [..., {B}] whose lanes are contiguous, got shape {tuple(t.shape)}")
        storage = t.untyped_storage()
        key = (storage.data_ptr(), kinds[t.dtype])
        if key not in self.keys:
            if len(self.keys) == MAX_SOURCES:
                raise ValueError(f"{who}: at most {MAX_SOURCES} source tensors are supported")
            self.keys.append(key)
            self.tensors.append(t)
            self.rows.append(storage.nbytes() // (t.element_size() * B))
        slot = self.keys.index(key)
        out = []
        for idx in np.ndindex(*t.shape[:-1]):
            offset = t.storage_offset() + sum(int(i) * int(s) for i, s in zip(idx, t.stride()[:-1]))
            if offset % B:
                raise ValueError(f"{who}: the view does not start on a row [{B}] of its tensor")
            out.append((slot, offset // B))
        return out


def _bounds(bound: Any, n: int, who: str) -> Tuple[np.ndarray, np.ndarray]:
    if bound is None:
        return np.zeros(n, dtype=bool), np.zeros(n)
    value = np.asarray(bound.detach().cpu().numpy() if hasattr(bound, "detach") else bound, dtype=np.float64).reshape(-1)
    if value.size not in (1, n):
        raise ValueError(f"{who}: expected one bound or one per element ({n}), got {value.size}")
    return np.ones(n, dtype=bool), np.broadcast_to(value, (n,)).copy()


def build_plan(reward: Any, terminations: Sequence[Termination], batch_size: int, dtype) -> ComposePlan:
    """The packed description of a reward tree (or None) and a list of terminations on tensors of `batch_size` lanes and the
    engine dtype `dtype`.  Raises what the reference raises and what the bounds of the kernel exclude."""
    src = _Sources(batch_size, dtype)
    nodes: List[Dict[str, Any]] = []
    child: List[int] = []
    weight: List[float] = []

    def add(c: Any, depth: int) -> int:
        if depth > MAX_DEPTH:
            raise ValueError(f"the reward tree is deeper than {MAX_DEPTH} levels")
        if len(nodes) == MAX_NODES:
            raise ValueError(f"at most {MAX_NODES} reward nodes are supported")
        n = len(nodes)
        node = dict(name=c.name, kind=LEAF, terminal=-1 if c.is_terminal is None else int(bool(c.is_terminal)),
                    normalized=int(bool(c.is_normalized)), slot=0, row=0, start=0, count=0, order=1.0)
        nodes.append(node)
        if isinstance(c, SurviveReward):
            node["kind"] = SURVIVE
        elif isinstance(c, RewardTerm):
            if not hasattr(c.row, "dim") or c.row.dim() != 1:
                raise ValueError(f"reward term '{c.name}': expected one row [{batch_size}] of a block tensor")
            ((node["slot"], node["row"]),) = src.locate(c.row, f"reward term '{c.name}'")
        elif isinstance(c, _Mixture):
            additive = isinstance(c, AdditiveMixtureReward)
            node["kind"] = ADDITIVE if additive else MULTIPLICATIVE
            node["order"] = c.order if additive else 1.0
            weights = c.weights if additive else (1.0,) * len(c.components)
            indices = [add(component, depth + 1) for component in c.components]
            node["start"], node["count"] = len(child), len(indices)
            child.extend(indices)
            weight.extend(weights)
        else:
            raise TypeError(f"expected a reward description, got {type(c).__name__}")
        return n

    if reward is not None:
        add(reward, 1)
    names = [n["name"] for n in nodes]
    for name in names:
        if names.count(name) > 1:
            # (bases/compositions.py:221-224)
            raise KeyError(f"Key '{name}' already reserved in 'info'. Impossible to store value of reward component.")
    terminations = list(terminations)
    if len(terminations) > MAX_CONDITIONS:
        raise ValueError(f"at most {MAX_CONDITIONS} termination conditions are supported, got {len(terminations)}")
    for t in terminations:
        if not isinstance(t, Termination):
            raise TypeError(f"expected a Termination, got {type(t).__name__}")
    cond_names = [t.name for t in terminations]
    if len(set(cond_names)) != len(cond_names):
        raise KeyError("two termination conditions share a name")
    conds, elems = [], []
    for t in terminations:
        who = f"termination '{t.name}'"
        cells = src.locate(t.rows, who)
        (has_low, low), (has_high, high) = _bounds(t.low, len(cells), who), _bounds(t.high, len(cells), who)
        if (has_low & has_high & (low > high)).any():
            raise ValueError(f"{who}: a low bound lies above its high bound")
        flags = (COND_ARRAY if t.rows.dim() >= 2 else 0) | (COND_TRUNCATION if t.is_truncation else 0) | \
                (COND_TRAINING_ONLY if t.training_only else 0)
        conds.append((len(elems), len(cells), flags, t.grace_period))
        elems += [(s, r, HAS_LOW * int(hl) + HAS_HIGH * int(hh), lo, hi) for (s, r), hl, lo, hh, hi in zip(cells, has_low, low, has_high, high)]
    if len(elems) > MAX_ELEMENTS:
        raise ValueError(f"at most {MAX_ELEMENTS} termination elements in total are supported, got {len(elems)}")
    col = lambda rows, k: [r[k] for r in rows]      # noqa: E731
    arrays = dict(
        source_kind=[k for _, k in src.keys], source_rows=src.rows,
        node_kind=[n["kind"] for n in nodes], node_terminal=[n["terminal"] for n in nodes],
        node_normalized=[n["normalized"] for n in nodes], node_slot=[n["slot"] for n in nodes], node_row=[n["row"] for n in nodes],
        node_child_start=[n["start"] for n in nodes], node_child_count=[n["count"] for n in nodes],
        node_order=[n["order"] for n in nodes], child=child, child_weight=weight,
        cond_elem_start=col(conds, 0), cond_elem_count=col(conds, 1), cond_flags=col(conds, 2), cond_grace=col(conds, 3),
        elem_slot=col(elems, 0), elem_row=col(elems, 1), elem_bounds=col(elems, 2), elem_low=col(elems, 3), elem_high=col(elems, 4))
    return ComposePlan(node_names=names, condition_names=cond_names, arrays=arrays, sources=list(src.tensors),
                       source_ptr=[p for p, _ in src.keys])
