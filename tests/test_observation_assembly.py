"""The observation assembly (jiminy_amd/csrc/jm_observe.h, jiminy_amd/observe.py, blocks.ObservationAssembler,
wrappers.AssembleObservation): `FlattenObservation(StackObservation(NormalizeObservation(ScaleObservation(
AdaptLayoutObservation(env)))))` as one kernel.

Host: the tables of the plan builder against the numpy restatement (tests/observe_numpy.py) and the numpy evaluation of the plan
against the chain of tensor wrappers, bit for bit; every refusal; the kernel body compiled for the host (tests/hostemu/observe)
against the numpy restatement, bit for bit in the three dtype pairs (IEEE basic operations only: no tolerance); the ABI.
Device: tile edges through the C ABI with guarded buffers; a stack sequence with skipped shifts and a lane reset against the chain
of tensor wrappers on the same device tensors; two ANYmal environments, one under `AssembleObservation`, one under the chain."""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from jiminy_amd import _abi, _lib, codegen, load_builtin, observe
from jiminy_amd import wrappers as W
from tests import observe_numpy as on
from tests.hostemu import observe as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
NEW_SYMBOLS = ("jm_observe_plan_create", "jm_observe_plan_destroy", "jm_block_observe")
PAIRS = [(np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32)]
PAIR_IDS = ["f64-f64", "f64-f32", "f32-f32"]
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------------------------- a small pipeline
def make_obs(B: int, dtype, device="cpu", seed: int = 0):
    """A nested observation like the environments': batch-first views of `[rows][B]` storage."""
    g = torch.Generator().manual_seed(seed)

    def leaf(*shape):
        return (4.0 * torch.rand((*shape, B), generator=g, dtype=torch.float64) - 2.0).to(dtype).to(device).movedim(-1, 0)
    return {"t": torch.zeros(B, dtype=dtype, device=device), "a": {"q": leaf(7), "v": leaf(6)}, "m": {"imu": leaf(2, 6)}}


SPEC = dict(layout=[(("x", "q"), ("a", "q", [(2, 7)])), (("x", "imu"), ("m", "imu", [(), (1, 4)])), (("y",), ("a", "v"))],
            nested_scale=[(("x",), 2.0), (("x", "q", [(1, 3)]), 4.0), (("y",), 0.5)],
            bounds={("x", "q"): (-1.0, 3.0)}, num_stack=3, nested_filter_keys=[("x",)])


def restated_plan(num_stack: int = 3) -> dict:
    """SPEC by hand.  Flat order: ('x', 'imu'), ('x', 'q'), ('y',); slots in the order the leaves are first used."""
    imu_rows = np.arange(12).reshape(2, 6)[:, 1:4].reshape(-1)
    leaves = [dict(slot=0, rows=imu_rows, mults=[[0.5]] * 6, mean=np.zeros(6), scale=np.ones(6), stacked=True),
              dict(slot=1, rows=np.arange(2, 7), mults=[[0.5], [0.5, 0.25], [0.5, 0.25], [0.5], [0.5]], mean=np.full(5, 1.0),
                   scale=np.full(5, 2.0), stacked=True),
              dict(slot=2, rows=np.arange(6), mults=[[2.0]] * 6, mean=np.zeros(6), scale=np.ones(6), stacked=False)]
    return on.make_plan([12, 7, 6], leaves, num_stack)


class Env:
    """The `reset / step / observation` surface over a fixed observation; `step` hands out the reset masks it is given."""

    def __init__(self, obs, engine=None) -> None:
        self.obs, self.engine, self.masks = obs, engine, []

    def observation(self):
        return self.obs

    def reset(self):
        return self.obs, {}

    def step(self, action):
        mask = self.masks.pop(0) if self.masks else None
        return self.obs, None, None, None, ({} if mask is None else {"reset_mask": mask})


def chain_of(env, spec: dict, dtype, skip_frames_ratio: int = -1):
    """The chain of tensor wrappers `AssembleObservation` stands for: the two new ones in front of the three of before."""
    chain = W.ScaleObservation(W.AdaptLayoutObservation(env, spec["layout"]), spec["nested_scale"])
    chain = W.StackObservation(W.NormalizeObservation(chain, spec["bounds"]), num_stack=spec["num_stack"],
                               nested_filter_keys=spec["nested_filter_keys"], skip_frames_ratio=skip_frames_ratio)
    return W.FlattenObservation(chain, dtype=dtype)


def test_plan_tables_equal_the_numpy_restatement():
    plan = observe.build_plan(make_obs(5, torch.float64), engine_dtype=torch.float64, dtype=torch.float32, **SPEC)
    want = restated_plan()
    assert plan.source_paths == [("m", "imu"), ("a", "q"), ("a", "v")] and plan.leaf_paths == [("x", "imu"), ("x", "q"), ("y",)]
    assert plan.leaf_stacked == [True, True, False] and (plan.n_elements, plan.n_positions) == (17, 39)
    for key in on.PLAN_KEYS:
        assert np.array_equal(np.asarray(plan.arrays[key]), np.asarray(want[key])), key
    assert same_bits(np.asarray(plan.arrays["multiplier"], dtype=np.float64), np.asarray(want["multiplier"], dtype=np.float64))
    # the flat order: a stacked leaf is [num_stack][elements], oldest first
    assert plan.arrays["pos_elem"][:18] == list(range(6)) * 3 and plan.arrays["pos_age"][:18] == [2] * 6 + [1] * 6 + [0] * 6
    assert plan.arrays["pos_elem"][33:] == list(range(11, 17)) and plan.arrays["pos_age"][33:] == [0] * 6
    desc, keep = plan.desc()
    emu.pack(desc)
    # ("t",) is left out by default, and kept on demand
    with_t = observe.build_plan(make_obs(5, torch.float64), engine_dtype=torch.float64, exclude=())
    assert with_t.leaf_paths[-1] == ("t",) and with_t.n_elements == 7 + 6 + 12 + 1 and with_t.num_stack == 1


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("skip", [-1, 1])
def test_plan_evaluates_to_the_chain_of_tensor_wrappers(pair, skip):
    """The numpy evaluation of the plan against the chain on the host: reset, four steps, a lane reset before the third launch."""
    dtype_in, dtype_out = pair
    B = 5
    obs = make_obs(B, TORCH[dtype_in])
    env = Env(obs)
    chain = chain_of(env, SPEC, TORCH[dtype_out], skip)
    plan = observe.build_plan(obs, engine_dtype=TORCH[dtype_in], dtype=TORCH[dtype_out], **SPEC)
    hist = np.zeros((3, plan.n_elements, B), dtype=dtype_in)
    mask = torch.tensor([True, False, False, True, False])
    env.masks = [None, mask, None, None]
    n_since = 0
    for launch in range(5):
        want = chain.reset()[0] if launch == 0 else chain.step(None)[0]
        shift = skip < 0 or n_since >= skip
        n_since = 0 if shift else n_since + 1
        sources = [np.ascontiguousarray(t.movedim(0, -1).numpy()) for t in observe.source_tensors(obs, plan)]
        got, hist = on.evaluate(plan.arrays, sources, hist, shift=shift and launch > 0, reset_mask=mask.numpy() if launch == 2 else None,
                                dtype_in=dtype_in, dtype_out=dtype_out)
        assert same_bits(got, want.numpy()), (launch, np.abs(got - want.numpy()).max())
        for t in observe.source_tensors(obs, plan):
            t.mul_(1.25).add_(0.1)


# ----------------------------------------------------------------------------------------------------------------- refusals
def _set(plan: dict, **changes) -> dict:
    new = {k: (list(v) if isinstance(v, list) else v) for k, v in plan.items()}
    new.update(changes)
    return new


def test_plan_builder_refusals():
    obs = make_obs(4, torch.float64)
    build = lambda o=obs, **kw: observe.build_plan(o, engine_dtype=torch.float64, **{**SPEC, **kw})      # noqa: E731
    many = {f"k{i:02d}": make_obs(4, torch.float64, seed=i)["a"]["v"] for i in range(17)}
    with pytest.raises(ValueError, match="1 to 16 sources are supported, got 17"):
        observe.build_plan(many, engine_dtype=torch.float64)
    assert len(observe.build_plan({k: v for k, v in list(many.items())[:16]}, engine_dtype=torch.float64).source_paths) == 16
    blocks = [(("y", [(0, 4)]), 2.0), (("y", [(1, 5)]), 3.0), (("y", [(2, 6)]), 5.0), (("y", [(3, 6)]), 7.0)]
    assert max(build(nested_scale=[(("y",), 1.5), (("y",), 2.5)] + blocks[:3]).arrays["elem_mult_count"]) == 4
    with pytest.raises(ValueError, match=r"element 3 of observation leaf \('y',\) has 5 multipliers, at most 4 per element"):
        build(nested_scale=[(("y",), 1.5)] + blocks)
    batch_major = dict(obs, a=dict(obs["a"], v=torch.zeros(4, 6, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"observation leaf \('a', 'v'\) is not a batch-first view of \[rows\]\[B\] storage"):
        build(batch_major)
    other_dtype = dict(obs, m={"imu": obs["m"]["imu"].float()})
    with pytest.raises(ValueError, match=r"observation leaf \('m', 'imu'\) is not a batch-first view .* in the engine dtype"):
        build(other_dtype)
    assert build(dict(batch_major, a=dict(batch_major["a"])), layout=[(("x", "q"), ("a", "q"))], nested_scale=None).n_elements == 7
    with pytest.raises(ValueError, match="must not be zero"):
        build(nested_scale=[(("y",), 0.0)])
    with pytest.raises(ValueError, match=r"observation leaf \('x', 'q'\) has a zero scale"):
        build(bounds={("x", "q"): (1.0, 1.0)})
    with pytest.raises(ValueError, match="The resulting observation space must not be empty."):
        build(layout=[])
    with pytest.raises(ValueError, match="Input nested keys must not be empty."):
        build(layout=[(("x",), ())])
    with pytest.raises(KeyError, match=r"Nested key '\('a', 'w'\)' is missing."):
        build(layout=[(("x",), ("a", "w"))])
    with pytest.raises(ValueError, match=r"Nested key \('z',\) not found in base observation space."):
        build(nested_scale=[(("z",), 2.0)])
    with pytest.raises(ValueError, match="float32 sources with a float64 output are not supported"):
        observe.build_plan(make_obs(4, torch.float32), engine_dtype=torch.float32, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"num_stack must be in \[1, 16\], got 17"):
        build(num_stack=17)
    with pytest.raises(ValueError, match="At least one observation leaf must be stacked."):
        build(nested_filter_keys=[("nope",)])
    wide = {"w": torch.zeros(2049, 2, dtype=torch.float64).T}
    with pytest.raises(ValueError, match="at most 2048 elements are supported, got 2049"):
        observe.build_plan(wide, engine_dtype=torch.float64)
    with pytest.raises(ValueError, match="1 to 8192 output positions are supported, got 10240"):
        observe.build_plan({"w": torch.zeros(2048, 2, dtype=torch.float64).T}, engine_dtype=torch.float64, num_stack=5)
    out = torch.zeros(4, 39)
    observe.check_no_alias(out, [("a leaf", obs["a"]["q"])])
    with pytest.raises(ValueError, match="out aliases a leaf"):
        observe.check_no_alias(obs["a"]["q"].movedim(0, -1)[3:], [("a leaf", obs["a"]["q"])])


def _rejections() -> list:
    good = restated_plan()
    return [
        (_set(good, source_rows=[1] * 17), "1 to 16 sources are supported, got 17"),
        (_set(good, elem_mult_count=[5] + good["elem_mult_count"][1:], multiplier=good["multiplier"] + [1.0] * 8),
         "element 0 has 5 multipliers, at most 4 per element are supported"),
        (_set(good, elem_scale=good["elem_scale"][:3] + [0.0] + good["elem_scale"][4:]), "element 3 has a zero scale"),
        (_set(good, num_stack=17), r"num_stack must be in \[1, 16\], got 17"),
        (_set(good, elem_slot=[], elem_row=[], elem_mult_start=[], elem_mult_count=[], elem_mean=[], elem_scale=[]),
         "The resulting observation space must not be empty."),
        (_set(good, elem_row=[12] + good["elem_row"][1:]), r"element 0 reads row 12, out of range \[0, 12\) of its slot"),
        (_set(good, elem_slot=[3] + good["elem_slot"][1:]), r"element 0 reads slot 3, out of range \[0, 3\)"),
        (_set(good, pos_age=[3] + good["pos_age"][1:]), r"position 0 has age 3, out of range \[0, 3\)"),
        (_set(good, pos_elem=good["pos_elem"][:-1] + [0], pos_age=good["pos_age"][:-1] + [0]), "repeats position 12"),
        (_set(good, pos_elem=good["pos_elem"][:-1], pos_age=good["pos_age"][:-1]), "element 16 is emitted at 0 ages"),
        (_set(good, pos_elem=good["pos_elem"][6:], pos_age=good["pos_age"][6:]), "element 0 is emitted at 2 ages"),
        (_set(good, elem_mean=[float("nan")] + good["elem_mean"][1:]), "element 0 has a mean or a scale that is not a number"),
    ]


def _big(D: int, W_: int, num_stack: int = 1) -> dict:
    return dict(source_rows=[1], elem_slot=[0] * D, elem_row=[0] * D, elem_mult_start=[0] * D, elem_mult_count=[0] * D, elem_mean=[0.0] * D,
                elem_scale=[1.0] * D, multiplier=[], num_stack=num_stack, pos_elem=[p % D for p in range(W_)],
                pos_age=[p // D for p in range(W_)])


def test_plan_validation_rejects_every_malformed_description():
    for plan in (restated_plan(), _big(2048, 2048), _big(512, 8192, 16)):
        d, keep = emu.plan_desc(plan)
        emu.pack(d)
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    for plan, message in _rejections():
        d, keep = emu.plan_desc(plan)
        with pytest.raises(ValueError, match=message):
            emu.pack(d)
    for plan, message in ((_big(2049, 2049), "at most 2048 elements are supported, got 2049"),
                          (_big(2048, 8193), "1 to 8192 output positions are supported, got 8193")):
        d, keep = emu.plan_desc(plan)
        with pytest.raises(ValueError, match=message):
            emu.pack(d)


def test_launch_refusals_on_the_host():
    plan, sources = on.synthetic_case(8, 6, 2)
    D, W_ = len(plan["elem_slot"]), len(plan["pos_elem"])
    src32 = [s.astype(np.float32) for s in sources]
    with pytest.raises(ValueError, match="float32 sources with a float64 output are not supported"):
        emu.run(plan, src32, np.zeros((2, D, 8), np.float32), np.zeros((8, W_)), dtype_in=np.float32, dtype_out=np.float64)
    # `out` that begins inside a source, inside the history: one buffer holds both
    n = sources[1].size
    joint = np.zeros(n + 8 * W_)
    inside = [sources[0], joint[:n].reshape(sources[1].shape), sources[2]]
    with pytest.raises(ValueError, match="out aliases source 1"):
        emu.run(plan, inside, np.zeros((2, D, 8)), joint[n - 1:n - 1 + 8 * W_].reshape(8, W_))
    emu.run(plan, inside, np.zeros((2, D, 8)), joint[n:].reshape(8, W_))         # (right behind it: no byte shared)
    n = 2 * D * 8
    joint = np.zeros(n + 8 * W_)
    with pytest.raises(ValueError, match="out aliases the history"):
        emu.run(plan, sources, joint[:n].reshape(2, D, 8), joint[n - 1:n - 1 + 8 * W_].reshape(8, W_))


# ------------------------------------------------------------------------------------------------------ the kernel body
SHAPES = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 130)]


def run_sequence(launch, plan: dict, sources, dtype_in, dtype_out, B: int):
    """Three launches -- a shift, a launch that does not shift with a lane reset, a shift -- of `launch(sources, shift, mask)
    -> (out, hist)` against the numpy restatement: `out` and the history bit for bit after each."""
    S, D = plan["num_stack"], len(plan["elem_slot"])
    hist = np.zeros((S, D, B), dtype=dtype_in)
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, B // 2, B - 1]] = 1
    for k, (shift, reset) in enumerate(((True, None), (False, mask), (True, None))):
        src = [(s + dtype_in(0.125 * k)).astype(dtype_in) for s in sources]
        want, hist = on.evaluate(plan, src, hist, shift=shift, reset_mask=reset, dtype_in=dtype_in, dtype_out=dtype_out)
        got, got_hist = launch(src, shift, reset)
        assert same_bits(got, want), (k, np.abs(got.astype(np.float64) - want).max())
        assert same_bits(got_hist, hist), k


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("num_stack", [1, 3])
def test_emulated_kernel_matches_the_numpy_restatement(pair, num_stack):
    dtype_in, dtype_out = pair
    for B, D in SHAPES:
        plan, sources = on.synthetic_case(B, D, num_stack)
        sources = [s.astype(dtype_in) for s in sources]
        assert set(plan["elem_mult_count"]) >= ({0} if D == 1 else {0, 1, 4})
        hist = np.zeros((num_stack, D, B), dtype=dtype_in)
        out = np.full((B, len(plan["pos_elem"])), 7.25, dtype=dtype_out)

        def launch(src, shift, reset):
            emu.run(plan, src, hist, out, shift=shift, reset_mask=reset, dtype_in=dtype_in, dtype_out=dtype_out)
            return out.copy(), hist.copy()
        run_sequence(launch, plan, sources, dtype_in, dtype_out, B)


# -------------------------------------------------------------------------------------------------------------------- ABI
def _prebuilt(model):
    path = codegen.lib_path(model)
    if not os.path.exists(path):
        pytest.skip(f"{os.path.basename(path)} not built (run __graft_entry__.build())")
    return _lib.load_for(model, allow_build=False)


def _last_error(lib) -> str:
    buf = C.create_string_buffer(1024)
    lib.L.jm_last_error(buf, 1024)
    return buf.value.decode()


def test_abi_version_symbols_and_structures():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    body = header.split("typedef struct jm_observe_desc")[1].split("} jm_observe_desc;")[0]
    order = [line.split(";")[0].split()[-1] for line in body.splitlines() if ";" in line]
    assert order == [f[0] for f in _abi.ObserveDesc._fields_]
    body = header.split("typedef struct jm_observe_io")[1].split("} jm_observe_io;")[0]
    order = [line.split(";")[0].split()[-1].split("[")[0] for line in body.splitlines() if ";" in line]
    assert order == list(_abi.OBSERVE_IO_FIELDS) and "const void * source[16];" in body and _abi.OBSERVE_MAX_SOURCES == 16
    # the sizes the host compiler gives the header's structures
    sizes = (C.c_int * 2)()
    emu._lib().emu_observe_sizes(sizes)
    assert list(sizes) == [C.sizeof(_abi.ObserveDesc), C.sizeof(_abi.ObserveIO)]
    assert "jm_observe.h" in open(os.path.join(ROOT, "jiminy_amd", "codegen.py")).read()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


def test_plan_create_validates_before_touching_the_device():
    """The rejections through the C ABI of a built library, on a machine without a device: JM_EINVAL and a message."""
    lib = _prebuilt(load_builtin("cartpole"))
    h = C.c_void_p()
    assert lib.L.jm_observe_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = emu.plan_desc(restated_plan())
    assert lib.L.jm_observe_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.pos_age = None
    assert lib.L.jm_observe_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)
    for plan, message in _rejections():
        d, keep_ = emu.plan_desc(plan)
        rc = lib.L.jm_observe_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value, message
        import re
        assert re.search(message, _last_error(lib)), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.ObserveIO()
    assert lib.L.jm_block_observe(None, _abi.JM_F64, _abi.JM_F64, 64, C.byref(io), 1, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


# ----------------------------------------------------------------------------------------------------------------- device
SENTINEL = -77.5


class DeviceObserve:
    """A plan on the device; `hist` and `out` live in buffers with a guard row filled with a sentinel on each side."""

    def __init__(self, lib, plan: dict, device, B: int, dtype_in, dtype_out):
        self.lib, self.device, self.plan, self.B = lib, device, plan, B
        self.dtype_in, self.dtype_out = dtype_in, dtype_out
        S, D, W_ = plan["num_stack"], len(plan["elem_slot"]), len(plan["pos_elem"])
        self.hist_buf = torch.full((S * D + 2, B), SENTINEL, dtype=TORCH[dtype_in], device=device)
        self.out_buf = torch.full((B + 2, W_), SENTINEL, dtype=TORCH[dtype_out], device=device)
        self.hist, self.out = self.hist_buf[1:-1].view(S, D, B), self.out_buf[1:-1]
        self.hist.zero_()
        desc, keep = emu.plan_desc(plan)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_observe_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_observe_plan_destroy(self.h)

    def run(self, sources, shift, reset):
        io, held = _abi.ObserveIO(), []
        put = lambda a: held.append(torch.as_tensor(np.ascontiguousarray(a), device=self.device)) or held[-1].data_ptr()      # noqa: E731
        for s, a in enumerate(sources):
            io.source[s] = put(a)
        io.reset_mask = None if reset is None else put(np.asarray(reset, dtype=np.uint8))
        io.hist, io.out = self.hist.data_ptr(), self.out.data_ptr()
        self.lib.check(self.lib.L.jm_block_observe(self.h, emu.code(self.dtype_in), emu.code(self.dtype_out), self.B, C.byref(io), int(shift),
                                                   C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        del held
        for buf in (self.hist_buf, self.out_buf):
            assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "a guard row was written"
        return self.out.cpu().numpy(), self.hist.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("num_stack", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}-D{d}" for b, d in SHAPES])
def test_device_tile_edges(shape, num_stack, pair, gpu_device):
    """Synthetic sources through the C ABI: 3 sources, multiplier chains of length 0, 1 and 4, stacked and unstacked leaves, at
    the edges of the 64 x 64 tile.  Outputs and history bit-equal to numpy, guard rows untouched."""
    (B, D), (dtype_in, dtype_out) = shape, pair
    plan, sources = on.synthetic_case(B, D, num_stack)
    dev = DeviceObserve(_prebuilt(load_builtin("cartpole")), plan, gpu_device, B, dtype_in, dtype_out)
    try:
        run_sequence(dev.run, plan, [s.astype(dtype_in) for s in sources], dtype_in, dtype_out, B)
    finally:
        dev.close()


def _engine(device, dtype, B: int):
    """What `blocks.ObservationAssembler` needs of an engine, over a prebuilt library."""
    return SimpleNamespace(_lib=_prebuilt(load_builtin("cartpole")), dtype=dtype, device=device, batch_size=B,
                           _stream=lambda: C.c_void_p(torch.cuda.current_stream(device).cuda_stream))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("skip", [-1, 1])
def test_device_stack_sequence_matches_the_chain_of_tensor_wrappers(skip, pair, gpu_device, monkeypatch):
    """Five launches at B = 130 (the reset and four steps), a lane reset before launch 3 on the lanes {0, 63, 64, 129}: after
    every launch `out` is bit-equal to `FlattenObservation(StackObservation(NormalizeObservation(...)))` of before, behind the
    tensor-program scale and layout wrappers, on the same device tensors."""
    monkeypatch.delenv("JIMINY_AMD_TENSOR_BLOCKS", raising=False)
    dtype_in, dtype_out = TORCH[pair[0]], TORCH[pair[1]]
    B = 130
    obs = make_obs(B, dtype_in, gpu_device)
    mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
    mask[[0, 63, 64, 129]] = True
    env, twin = Env(obs, _engine(gpu_device, dtype_in, B)), Env(obs)
    env.masks, twin.masks = [None, mask, None, None], [None, mask, None, None]
    fused = W.AssembleObservation(env, dtype=dtype_out, skip_frames_ratio=skip, **SPEC)
    chain = chain_of(twin, SPEC, dtype_out, skip)
    for launch in range(5):
        got = fused.reset()[0] if launch == 0 else fused.step(None)[0]
        want = chain.reset()[0] if launch == 0 else chain.step(None)[0]
        assert got.dtype == dtype_out and got.shape == (B, 39) and got is fused.observation()
        assert torch.equal(got, want), (launch, float((got - want).abs().max()))
        for t in (obs["a"]["q"], obs["a"]["v"], obs["m"]["imu"]):
            t.mul_(1.25).add_(0.1)


@pytest.mark.gpu
def test_environment_under_the_assembled_observation(gpu_device, monkeypatch):
    """Two ANYmal environments of 64 lanes, same seed, same actions, four steps with auto-reset (every lane is truncated after
    the second): one under `AssembleObservation` with a layout, scales, bounds and a stack of 3, one under the chain of tensor
    wrappers.  The observations are bit-equal at reset and after every step, and `AssembleObservation.step` dispatches no tensor
    operation on top of the environment's but views."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from jiminy_amd.envs import make_anymal_env
    monkeypatch.delenv("JIMINY_AMD_TENSOR_BLOCKS", raising=False)
    spec = dict(layout=[(("joints", "q"), ("states", "agent", "q", [(7, 19)])), (("joints", "v"), ("states", "agent", "v", [(6, 18)])),
                        (("base", "twist"), ("states", "agent", "v", [(0, 6)])), (("imu",), ("measurements", "ImuSensor")),
                        (("targets",), ("actions", "pd_controller", [0, ()]))],
                nested_scale=[(("joints",), 2.0), (("joints", "v"), 4.0), (("base", "twist", [(3, 6)]), 8.0), (("imu",), 9.81)],
                bounds={("joints", "q"): (-3.0, 3.0), ("targets",): (-2.0, 2.5)}, num_stack=3, nested_filter_keys=[("joints",), ("imu",)])
    envs = [make_anymal_env(64, device=gpu_device, simulation_duration_max=0.07) for _ in range(2)]
    fused = W.AssembleObservation(envs[0], dtype=torch.float32, **spec)
    chain = chain_of(envs[1], spec, torch.float32)
    got, want = fused.reset(seed=5)[0], chain.reset(seed=5)[0]
    n_imu = envs[0].observation()["measurements"]["ImuSensor"][0].numel()
    assert got.dtype == torch.float32 and got.shape == want.shape == (64, 3 * (12 + 12 + n_imu) + 6 + 12)
    assert torch.equal(got, want)
    g = torch.Generator(device="cpu").manual_seed(0)
    n_resets = 0
    for step in range(4):
        action = (0.2 * torch.rand(64, 12, generator=g, dtype=torch.float64) - 0.1).to(gpu_device)
        a, b = fused.step(action), chain.step(action)
        assert torch.equal(a[0], b[0]), (step, float((a[0] - b[0]).abs().max()))
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        n_resets += int("reset_mask" in a[4])
        assert bool(torch.isfinite(a[0]).all())
    assert n_resets == 2

    log, span = [], []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            log.append(func)
            return func(*args, **(kwargs or {}))
    inner = envs[0].step

    def marked(action):
        span.append(len(log))
        out = inner(action)
        span.append(len(log))
        return out
    monkeypatch.setattr(envs[0], "step", marked)
    with Record():
        for _ in range(2):          # (the second of them resets the lanes: the step hands over `info["reset_mask"]`)
            fused.step(action)
    assert len(span) == 4 and span[1] > span[0]
    extra = log[:span[0]] + log[span[1]:span[2]] + log[span[3]:]
    print("tensor operations of AssembleObservation.step outside env.step:", [str(f) for f in extra])
    assert all(f.is_view for f in extra), [str(f) for f in extra if not f.is_view]
