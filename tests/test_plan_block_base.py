"""The base of the plan-backed blocks (`jiminy_amd.blocks._PlanBlock`): the life of a plan against a fake library, the one
tensor check, the one mask normalisation, the table of plan families, and on the device one rebuild of two blocks."""
import contextlib
import gc
import os
from types import SimpleNamespace

import pytest
import torch

from jiminy_amd import _abi, _lib, blocks

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jiminy_hip.h")
FAMILIES = ("deform", "attitude", "frames", "locomotion", "actuation", "footposes", "tracking", "trajectory", "centroidal",
            "trackrewards", "support", "compose", "observe")
TENSOR_MESSAGE = "pipeline block tensors must be contiguous engine-dtype tensors on the engine's device"
HANDLE = 0x5EED


class FakeLibrary:
    """Stands for `HipLibrary.L`: records every call by name; a create writes `HANDLE` unless `fail_create`."""

    def __init__(self, fail_create: bool = False) -> None:
        self.calls, self.fail_create = [], fail_create

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name.endswith("_plan_create"):
                if self.fail_create:
                    return _abi.JM_EINVAL
                args[1]._obj.value = HANDLE
            return _abi.JM_OK
        return call

    def names(self):
        return [name for name, _ in self.calls]


def fake_engine(L=None, device="cpu", dtype=torch.float64, batch_size=4):
    def check(rc):
        if rc != _abi.JM_OK:
            raise ValueError("create refused")
    return SimpleNamespace(dtype=dtype, device=torch.device(device), batch_size=batch_size, _lib=SimpleNamespace(L=L, check=check))


class Block(blocks._PlanBlock):
    def __init__(self, engine, plan, family="frames", raise_first=False) -> None:
        if raise_first:
            raise ValueError("refused before anything was bound")
        self._bind(engine)
        self.plan = plan
        self._create_plan(family)


def stub_plan(desc_type=_abi.FramesDesc):
    return SimpleNamespace(desc=lambda: (desc_type(), ["kept alive until the library copied it"]))


@pytest.fixture
def no_device(monkeypatch):
    """`torch.cuda.device(...)` of `_create_plan` selects the engine's GPU; the fake engines have none."""
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())


def test_lifecycle_against_a_fake_library(no_device):
    L = FakeLibrary()
    block = Block(fake_engine(L), stub_plan())
    assert L.names() == ["jm_frames_plan_create"] and block._plan.value == HANDLE
    desc_ref, handle_ref = L.calls[0][1]
    assert isinstance(desc_ref._obj, _abi.FramesDesc) and handle_ref._obj is block._plan
    del block, desc_ref, handle_ref
    gc.collect()
    assert L.names() == ["jm_frames_plan_create", "jm_frames_plan_destroy"]
    assert L.calls[1][1][0].value == HANDLE
    # a second explicit __del__ is a no-op
    L = FakeLibrary()
    block = Block(fake_engine(L), stub_plan(_abi.SupportDesc), family="support")
    block.__del__()
    block.__del__()
    del block
    gc.collect()
    assert L.names() == ["jm_support_plan_create", "jm_support_plan_destroy"]
    # create returned an error through `check`: the constructor raises and nothing is destroyed
    L = FakeLibrary(fail_create=True)
    with pytest.raises(ValueError, match="create refused"):
        Block(fake_engine(L), stub_plan())
    gc.collect()
    assert L.names() == ["jm_frames_plan_create"]
    # a family the table does not hold never reaches the library
    L = FakeLibrary()
    with pytest.raises(AssertionError):
        Block(fake_engine(L), stub_plan(), family="nothing")
    gc.collect()
    assert L.calls == []


def test_del_is_safe_on_a_half_built_block():
    with pytest.raises(ValueError, match="refused before anything was bound"):
        Block(None, None, raise_first=True)
    half = Block.__new__(Block)
    half.__del__()                      # before `_bind`: no `_plan`, no `_L`
    half.__del__()
    bound = Block.__new__(Block)
    bound._bind(fake_engine(FakeLibrary()))
    bound.__del__()                     # before `_create_plan`
    assert bound._L.calls == []
    # a destroy that raises (the library is gone at interpreter shutdown) is swallowed, and not tried again
    broken = Block.__new__(Block)
    broken._bind(fake_engine(None))     # `None.jm_frames_plan_destroy` raises AttributeError
    broken._family, broken._plan = "frames", broken._C.c_void_p(HANDLE)
    broken.__del__()
    assert broken._plan is None


def test_ptr_checks_once_for_every_block():
    eng = fake_engine()
    block = Block.__new__(Block)
    block._bind(eng)
    good = torch.zeros(3, 4, dtype=torch.float64)
    assert block._ptr(good) == good.data_ptr() and block._ptr(None) is None
    assert block._dtype == _abi.JM_F64
    for bad in (good.t(), good.float(), torch.zeros(3, 4, dtype=torch.float64, device="meta"), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError) as err:
            block._ptr(bad)
        assert str(err.value) == TENSOR_MESSAGE
    counts = torch.zeros(4, dtype=torch.int32)
    assert block._ptr(counts, torch.int32) == counts.data_ptr()
    with pytest.raises(ValueError):
        block._ptr(good, torch.int32)
    # a tensor without elements is a null pointer (`FootPoseQuantities` with one foot), after the same check
    assert block._ptr(torch.zeros(7, 0, 4, dtype=torch.float64)) is None
    assert block._ptr(good[:, :0]) is None
    with pytest.raises(ValueError):
        block._ptr(torch.zeros(7, 0, 4, dtype=torch.float32))
    # float32 engines: the dtype code and the check follow the engine
    single = Block.__new__(Block)
    single._bind(fake_engine(dtype=torch.float32))
    assert single._dtype == _abi.JM_F32 and single._ptr(good.float().contiguous()) is not None
    with pytest.raises(ValueError):
        single._ptr(good)
    # the per-tick blocks share the check
    assert blocks.HipBlocks._ptr is blocks._PlanBlock._ptr and blocks.MahonyFilter._ptr is blocks._PlanBlock._ptr


def test_mask_normalises_every_dtype():
    B = 5
    block = Block.__new__(Block)
    block._bind(fake_engine(batch_size=B))
    assert block._mask(None) is None
    want = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    for dtype in (torch.bool, torch.uint8, torch.int64):
        mask = block._mask(want.to(dtype))
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (B,) and mask.is_contiguous() and torch.equal(mask, want)
    strided = torch.tensor([1, 9, 0, 9, 0, 9, 1, 9, 0, 9], dtype=torch.int64)[::2]
    mask = block._mask(strided)
    assert mask.is_contiguous() and torch.equal(mask, want)
    with pytest.raises(ValueError) as err:
        block._mask(torch.zeros(B + 1, dtype=torch.bool))
    assert str(err.value) == f"lane_mask must have shape ({B},)"
    # the strict flags of `Composition.refresh` / `ObservationAssembler.refresh` convert nothing
    flags = torch.tensor([True, False, False, True, False])
    assert block._flags(flags, "reset_mask").data_ptr() == flags.data_ptr() and block._flags(None, "reset_mask") is None
    for bad in (want.to(torch.int64), torch.zeros(B + 1, dtype=torch.bool), torch.zeros(2 * B, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError, match=f"reset_mask must be a contiguous bool or uint8 tensor of shape \\({B},\\)"):
            block._flags(bad, "reset_mask")


def test_family_table_drives_the_abi():
    assert tuple(_abi.PLAN_FAMILIES) == FAMILIES
    assert isinstance(_lib.ABI_SYMBOLS, tuple) and len(set(_lib.ABI_SYMBOLS)) == len(_lib.ABI_SYMBOLS)
    header = open(HEADER).read()
    for family, desc in _abi.PLAN_FAMILIES.items():
        assert issubclass(desc, _abi.C.Structure)
        for op in ("create", "destroy"):
            name = f"jm_{family}_plan_{op}"
            assert name in _lib.ABI_SYMBOLS and f"int32_t {name}(" in header, name
        assert f"int32_t jm_{family}_plan_create(const jm_{family}_desc * desc, jm_{family}_plan ** out)" in " ".join(header.split())
    # the thirteen blocks are the subclasses of the base, one per family
    assert len([c for c in blocks._PlanBlock.__subclasses__() if c.__module__ == blocks.__name__]) == len(FAMILIES)


@pytest.mark.gpu
def test_rebuilt_blocks_give_the_same_bits(gpu_device):
    """ANYmal at B = 65 (one full wavefront and a one-lane tail): `FrameKinematics` and `LocomotionQuantities` built, reset,
    stepped once and refreshed; dropped; built again on the same engine from the same state: every output bit for bit.  Then
    a masked reset with an int64 mask of lane 64 alone leaves lanes 0-63 bit for bit."""
    from jiminy_amd import load_builtin
    from jiminy_amd.engine import BatchedEngine
    from jiminy_amd.synthetic import sample_states
    model, B, dt = load_builtin("anymal"), 65, 1e-3
    st = sample_states(model, B, seed=1)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("contact_forces", "centroidal"))
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt},
                     "contacts": {"model": "spring_damper"}})
    eng.set_command(torch.from_numpy(st["command"]))
    names = ["root_joint"] + list(model.contacts)
    frame_outputs = ("pose", "velocity", "average_velocity", "pose_mean", "quat_no_yaw", "pose_prev")
    loco_outputs = ("com", "vcom", "odom_pose", "zmp", "dcm", "h_angular", "scalars")

    def one_pass():
        eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
        fk = blocks.FrameKinematics(eng, names, average=True)
        lq = blocks.LocomotionQuantities(eng, fk, forces=False, momentum_cutoff=1.0)
        fk.reset()
        lq.reset()
        eng.step(dt)
        fk.refresh()
        fk.refresh_average(dt)
        lq.refresh()
        out = {k: getattr(fk, k).clone() for k in frame_outputs}
        out.update({k: getattr(lq, k).clone() for k in loco_outputs})
        return fk, lq, out
    fk, lq, first = one_pass()
    torch.cuda.synchronize(gpu_device)
    eng.stop()
    del fk, lq
    gc.collect()
    fk, lq, second = one_pass()
    assert (fk._family, lq._family) == ("frames", "locomotion") and fk._plan and lq._plan
    for k, t in first.items():        # (bits, not values: the ZMP of a robot in free fall is NaN)
        assert torch.equal(second[k].view(torch.int64), t.view(torch.int64)), k
    for k in ("pose", "average_velocity", "com", "dcm"):
        assert bool(torch.isfinite(first[k]).all()) and float(first[k].abs().max()) > 0.0, k
    # masked reset: an int64 mask that selects the tail lane only
    mask = torch.zeros(B, dtype=torch.int64, device=gpu_device)
    mask[64] = 1
    tensors = {k: getattr(fk, k) for k in frame_outputs[:2] + ("pose_prev",)}
    tensors.update({k: getattr(lq, k) for k in loco_outputs})
    for t in tensors.values():
        t.fill_(7.25)
    fk.reset(mask)
    lq.reset(mask)
    for k, t in tensors.items():
        assert torch.equal(t[..., :64], torch.full_like(t[..., :64], 7.25)), k
        assert not bool((t[..., 64] == 7.25).all()), k
    with pytest.raises(ValueError, match="lane_mask must have shape \\(65,\\)"):
        fk.reset(mask[:64])
    eng.stop()
