"""Host side of the `DeformationEstimator` observer block: from a `CompiledModel` and the names of its IMU and
flexibility frames to the plan `jm_block_deformation_estimator` interprets on the device.

Reference: python/gym_jiminy/common/gym_jiminy/common/blocks/deformation_estimator.py --
`get_flexibility_imu_frame_chains` (:238-413) decides which flexibility points are observable from which IMUs and in
which order; `DeformationEstimator.__init__` / `_setup` (:501-817) turn that into index lists and pick, for every
flexibility point, the frame of the theoretical (rigid) model whose rotation stands for it (:776-788).  The chain
extraction is restated here from its behaviour (tests compare it with recorded outputs of the reference function,
tests/golden/ref_deformation.npz), including the order it walks the tree in: from the leaves to the root.

The theoretical kinematics need no second model: the compiled (extended) model with every spherical joint at the
identity and every backlash joint at zero has the rigid model's frame rotations (a flexibility joint is inserted at the
joint's placement, model.py `build_model_from_urdf`).  A free-flyer root sits at the identity (:566-570).

One deviation from the reference: `flex_frame_names` must name frames at which the compiled model HAS a flexibility
joint (`NotImplementedError` otherwise).  The reference accepts any frame, by building a throw-away flexible model from
the URDF; a `CompiledModel` does not keep the URDF.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from ._plan import AXIS_KIND, SEG_AXIS, SEG_NONE, SEG_X, SEG_Y, SEG_Z, SegmentTable, fill_desc  # noqa: F401 (kinds of jm_deform_desc)
from .model import (BACKLASH_JOINT_SUFFIX, FLEXIBLE_JOINT_SUFFIX, JT_FREEFLYER, JT_RUBU, JT_RUBX, JT_RUBY, JT_RUBZ, JT_SPHERICAL,
                    CompiledModel)

Chain = Tuple[List[str], List[Optional[str]], List[bool]]


def flexibility_imu_frame_chains(parents: Sequence[int], root_is_free: bool, flex_joint_of: Dict[str, int],
                                 imu_joint_of: Dict[str, int]) -> List[Chain]:
    """≙ `get_flexibility_imu_frame_chains` (deformation_estimator.py:238-413) on a bare tree: `parents[j]` is the parent
    of joint j (joint 0 = universe, `parents[0] = 0`), `root_is_free` says whether joint 1 is a free-flyer, the two
    dictionaries give the joint every flexibility joint name / IMU frame name is attached to.

    Returns `[(flexibility names, IMU names (None where missing), flipped flags), ...]`, one entry per contiguous chain
    of interleaved IMUs and flexibility points.  Chains run from a leaf towards the root (and down again to another
    leaf where two branches meet), so a fixed-base chain has its missing IMU at the LAST position."""
    n = len(parents)
    leaves = [j for j in range(n) if j not in set(int(p) for p in parents)]
    supports = []
    for leaf in leaves:
        path, j = [leaf], leaf
        while j != 0:
            j = int(parents[j])
            path.append(j)
        supports.append(path)
    # every pair of supports makes one chain: up the first to the first joint they share, down the second
    chains = []
    for i, up in enumerate(supports):
        for down in supports[i + 1:]:
            meet = next(j for j in up if j in down)
            chains.append(up[:up.index(meet) + 1] + down[:down.index(meet)][::-1])
    if not chains:
        chains.append(supports[0])

    flex_name = {j: name for name, j in flex_joint_of.items()}
    imu_name = {j: name for name, j in imu_joint_of.items()}
    flex_joints, imu_joints = set(flex_name), set(imu_name)
    if not root_is_free:
        if 1 in imu_joints:
            raise ValueError("There must not be an IMU frame attached to the root joint of "
                             "the robot if it has a fixed based (no freeflyer).")
        if not imu_joints.issuperset(leaves):
            raise ValueError("There must be an IMU frame attached to all the leaf joints "
                             "of the robot if it has a fixed based (no freeflyer).")

    # keep the joints that matter; a joint that is both appears twice (its flexibility point and its IMU)
    both, imu_only = flex_joints & imu_joints, imu_joints - flex_joints
    doubled_chains = []
    for chain in chains:
        kept = [j for j in chain if j in flex_joints or j in imu_joints]
        if len(kept) < 2:
            continue
        doubled, expect_flex = [], False
        for j in kept:
            doubled.append(j)
            if j in both:
                doubled.append(j)
            elif (expect_flex and j in flex_joints) or (not expect_flex and j in imu_joints):
                expect_flex = not expect_flex
            else:
                raise ValueError("Flexibility and IMU frames must interleave.")
        doubled_chains.append(doubled)

    # (parent IMU, flexibility, child IMU) triplets; None at an end without IMU
    triplets: List[List[Optional[int]]] = []
    for chain in doubled_chains:
        if chain[0] not in imu_only:
            triplets.append([None, chain[0], chain[1]])
        for k in range(0, len(chain) - 2, 2):
            triplets.append(list(chain[k:k + 3]))
        if chain[-1] not in imu_only:
            triplets.append([chain[-2], chain[-1], None])
    # one triplet per flexibility point, a complete one preferred over an orphan one
    kept_triplets: List[List[Optional[int]]] = []
    for t in triplets:
        orphan = t[0] is None or t[2] is None
        seen = [k[1] for k in kept_triplets]
        if t[1] not in seen:
            kept_triplets.append(t)
        elif not orphan:
            at = seen.index(t[1])
            if kept_triplets[at][0] is None or kept_triplets[at][2] is None:
                kept_triplets[at] = t

    out: List[Chain] = []
    previous_child: Optional[int] = -1
    for parent, flex, child in kept_triplets:
        if parent is None:
            flipped = flex >= child
        elif child is None:
            flipped = parent >= flex
        else:
            flipped = [parent, flex, child] != sorted([parent, flex, child])
        if previous_child != parent:
            out.append(([], [imu_name.get(parent)], []))
        previous_child = child
        out[-1][0].append(flex_name[flex])
        out[-1][1].append(imu_name.get(child))
        out[-1][2].append(bool(flipped))
    return out


def _is_backlash(model: CompiledModel, j: int) -> bool:
    name = model.joint_names[j]
    return name.endswith(BACKLASH_JOINT_SUFFIX) and name[:-len(BACKLASH_JOINT_SUFFIX)] in model.joint_names


def _flexibility_joint(model: CompiledModel, frame_name: str) -> int:
    """Index of the spherical joint the compiled model has at frame `frame_name` (in front of the mechanical joint of
    that name, or in place of the fixed joint of that name)."""
    for name in (frame_name + FLEXIBLE_JOINT_SUFFIX, frame_name):
        if name in model.joint_names and int(model.jtypes[model.joint_names.index(name)]) == JT_SPHERICAL:
            return model.joint_names.index(name)
    model.frame(frame_name)     # LookupError for a frame that does not exist at all
    raise NotImplementedError(f"The compiled model has no flexibility joint at frame '{frame_name}': build it with this "
                              "frame in its `flexibility` list (the reference inserts one in a throw-away model).")


@dataclass
class DeformationPlan:
    """What `DeformationEstimator.__init__` / `_setup` of the reference work out, plus the arrays of `jm_deform_desc`."""
    chains: List[Chain]                          # ≙ `flex_imu_frame_names_chains`
    flexibility_frame_names: List[str]           # re-ordered (:613-616): the columns of the outputs
    is_chain_orphan: List[Tuple[bool, bool]]
    imu_indices: List[Tuple[int, ...]]           # ≙ `_obs_imu_indices`
    parent_flex_joint_names: List[str]           # joint whose theoretical frame stands for each flexibility point (:776-788)
    ignore_twist: bool
    compute_rpy: bool
    arrays: Dict[str, Any] = field(default_factory=dict)

    @property
    def n_flex(self) -> int:
        return len(self.flexibility_frame_names)

    def desc(self) -> Tuple["_abi.DeformDesc", List[np.ndarray]]:
        return make_desc(**self.arrays)


def make_desc(*, n_imu: int, n_enc: int, ignore_twist: bool, chain_nflex, chain_orphan, chain_imu, chain_imu_frame, flex_frame,
              flex_flipped, frame_seg_start, seg_kind, seg_enc, seg_rot, seg_axis, seg_ratio) -> Tuple["_abi.DeformDesc", List[np.ndarray]]:
    """`jm_deform_desc` from plain arrays (layout: include/jiminy_hip.h); the second value keeps them alive."""
    d = _abi.DeformDesc()
    a, keep = fill_desc(d, dict(chain_nflex=chain_nflex, chain_orphan=chain_orphan, chain_imu=chain_imu,
                                chain_imu_frame=chain_imu_frame, flex_frame=flex_frame, flex_flipped=flex_flipped,
                                frame_seg_start=frame_seg_start, seg_kind=seg_kind, seg_enc=seg_enc),
                        dict(seg_rot=seg_rot, seg_axis=seg_axis, seg_ratio=seg_ratio))
    d.n_imu, d.n_enc, d.ignore_twist = int(n_imu), int(n_enc), int(bool(ignore_twist))
    d.n_chain, d.n_flex = len(a["chain_nflex"]), len(a["flex_frame"])
    d.n_frame, d.n_seg = len(a["frame_seg_start"]) - 1, len(a["seg_kind"])
    return d, keep


def build_plan(model: CompiledModel, imu_frame_names: Sequence[str], flex_frame_names: Sequence[str],
               ignore_twist: bool = True, compute_rpy: bool = True) -> DeformationPlan:
    """≙ `DeformationEstimator.__init__` + `_setup` (deformation_estimator.py:501-817) for a compiled model."""
    if not imu_frame_names or not flex_frame_names:
        raise RuntimeError("Please specify at least one IMU and one deformation point.")
    imu_frame_names, flex_frame_names = list(imu_frame_names), list(flex_frame_names)

    flex_joint_of = {model.joint_names[_flexibility_joint(model, name)]: _flexibility_joint(model, name) for name in flex_frame_names}
    flex_joint_names = list(flex_joint_of)
    imu_joint_of = {name: int(model.frame(name).parent_joint) for name in imu_frame_names}
    raw = flexibility_imu_frame_chains([int(p) for p in model.parents], bool(model.has_freeflyer), flex_joint_of, imu_joint_of)
    # flexibility joint names back to the frames the user named (:596-604)
    chains: List[Chain] = [([flex_frame_names[flex_joint_names.index(n)] for n in flexs], imus, flipped)
                           for flexs, imus, flipped in raw]
    if model.has_freeflyer and any(None in imus for _, imus, _ in chains):
        raise NotImplementedError("Freeflyer estimator is not supported for now.")

    # encoders: one per mechanical joint, none on an unbounded revolute joint (:678-695)
    encoders = model.sensors.get("EncoderSensor", [])
    mechanical = [j for j in range(1, model.njoints)
                  if int(model.jtypes[j]) not in (JT_FREEFLYER, JT_SPHERICAL) and not _is_backlash(model, j)]
    if len(encoders) < len(mechanical):
        raise ValueError("The robot must have one encoder per mechanical joints.")
    encoder_of: Dict[int, Tuple[int, float]] = {}
    for i, s in enumerate(encoders):
        if int(model.jtypes[s["joint"]]) in (JT_RUBX, JT_RUBY, JT_RUBZ, JT_RUBU):
            raise ValueError("Revolute unbounded joints are not supported for now.")
        encoder_of[int(s["joint"])] = (i, 1.0 if s["joint_side"] else 1.0 / float(s["reduction"]))
    imu_sensor_of = {s["frame"]: i for i, s in enumerate(model.sensors.get("ImuSensor", []))}

    # frames of the theoretical model, as segment lists
    segs = SegmentTable()

    def joint_segment(j: int):
        # (prismatic joints do not rotate; spherical, backlash and free-flyer joints sit at the identity)
        t = int(model.jtypes[j])
        if t not in AXIS_KIND or _is_backlash(model, j):
            return None
        if j not in encoder_of:
            raise ValueError("The robot must have one encoder per mechanical joints.")
        return AXIS_KIND[t], encoder_of[j][0], model.axes[j], encoder_of[j][1]

    chain_nflex, chain_orphan, chain_imu, chain_imu_frame, flex_frame, flex_flipped = [], [], [], [], [], []
    imu_indices, parent_names, orphans = [], [], []
    for flexs, imus, flipped in chains:
        orphan = (imus[0] is None, imus[-1] is None)
        if orphan[0]:
            # (cannot be reached: a fixed base has its missing IMU at the last position, a free-flyer raised above)
            raise NotImplementedError("A chain of flexibility points without IMU in front of its first one is not supported.")
        orphans.append(orphan)
        chain_nflex.append(len(flexs))
        chain_orphan.append([int(orphan[0]), int(orphan[1])])
        indices = []
        for name in filter(None, imus):
            if name not in imu_sensor_of:
                raise KeyError(name)
            indices.append(imu_sensor_of[name])
            fr = model.frame(name)
            chain_imu.append(imu_sensor_of[name])
            chain_imu_frame.append(segs.add_frame(model, int(fr.parent_joint), fr.R, joint_segment))
        imu_indices.append(tuple(indices))
        for name, flip in zip(flexs, flipped):
            # nearest ancestor joint that belongs to the theoretical model and is not a flexibility (:776-788)
            j = int(model.parents[_flexibility_joint(model, name)])
            while j != 0 and (int(model.jtypes[j]) == JT_SPHERICAL or _is_backlash(model, j)):
                j = int(model.parents[j])
            parent_names.append(model.joint_names[j])
            flex_frame.append(segs.add_frame(model, j, np.eye(3), joint_segment))
            flex_flipped.append(int(flip))

    arrays = dict(n_imu=len(model.sensors.get("ImuSensor", [])), n_enc=len(encoders), ignore_twist=bool(ignore_twist),
                  chain_nflex=chain_nflex, chain_orphan=chain_orphan, chain_imu=chain_imu, chain_imu_frame=chain_imu_frame,
                  flex_frame=flex_frame, flex_flipped=flex_flipped, frame_seg_start=segs.frame_seg_start, seg_kind=segs.kind,
                  seg_enc=segs.index, seg_rot=np.array(segs.rot), seg_axis=np.array(segs.axis), seg_ratio=segs.ratio)
    return DeformationPlan(chains=chains, flexibility_frame_names=[n for flexs, _, _ in chains for n in flexs],
                           is_chain_orphan=orphans, imu_indices=imu_indices, parent_flex_joint_names=parent_names,
                           ignore_twist=bool(ignore_twist), compute_rpy=bool(compute_rpy), arrays=arrays)
