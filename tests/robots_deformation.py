"""The flexible arm authored for the DeformationEstimator tests (tests/data/flex_arm.urdf) and its variants."""
from __future__ import annotations

import os
import tempfile
from typing import List

import numpy as np

from jiminy_amd.model import CompiledModel, add_motor, add_sensor, build_model_from_urdf

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
FLEX_FRAMES = ("f12", "f23", "elbow", "f45")
# the placement `flex_arm(rotated_placement=True)` gives the flexibility frame f23 (roll-pitch-yaw of the fixed joint's origin)
ROTATED_F23_RPY = (0.4, -0.3, 0.6)


def flex_arm(has_freeflyer: bool = False, rotated_placement: bool = False, stiffness: float = 400.0, damping: float = 4.0,
             flex_inertia: float = 1e-2, continuous_elbow: bool = False) -> CompiledModel:
    """Fixed base: IMUs imu2 .. imu5 behind the four flexibility points, none in front of the first one (the base is where
    the real robot IS the theoretical one).  Free-flyer: imu0 on the root body as well.  The sensors are attached in an
    order that is not the chain's.  `rotated_placement`: the flexibility frame f23 is rotated against its parent joint; `continuous_elbow`: the elbow is an
    unbounded revolute joint (which the block refuses)."""
    path = os.path.join(DATA, "flex_arm.urdf")
    tmp = None
    if rotated_placement or continuous_elbow:
        text = open(path).read()
        old = '<joint name="f23" type="fixed">\n    <origin xyz="0.25 0 0" rpy="0 0 0"/>'
        assert old in text and '<joint name="elbow" type="revolute">' in text
        if rotated_placement:
            text = text.replace(old, '<joint name="f23" type="fixed">\n    <origin xyz="0.25 0 0" rpy="%g %g %g"/>' % ROTATED_F23_RPY)
        if continuous_elbow:
            text = text.replace('<joint name="elbow" type="revolute">', '<joint name="elbow" type="continuous">')
        tmp = tempfile.NamedTemporaryFile("w", suffix=".urdf", delete=False)
        tmp.write(text)
        tmp.close()
        path = tmp.name
    name = "flex_arm" + ("_ff" if has_freeflyer else "") + ("_rot" if rotated_placement else "") + ("_cont" if continuous_elbow else "")
    try:
        m = build_model_from_urdf(path, has_freeflyer=has_freeflyer, name=name, flexibility=[
            {"frameName": f, "stiffness": stiffness * np.ones(3), "damping": damping * np.ones(3),
             "inertia": flex_inertia * np.ones(3)} for f in FLEX_FRAMES])
    finally:
        if tmp is not None:
            os.unlink(tmp.name)
    add_motor(m, "shoulder", "shoulder", mechanicalReduction=10.0, enableVelocityLimit=False, enableEffortLimit=False)
    add_motor(m, "elbow", "elbow", enableVelocityLimit=False, enableEffortLimit=False)
    add_sensor(m, "EncoderSensor", "elbow", motor_name="elbow")
    add_sensor(m, "EncoderSensor", "shoulder", motor_name="shoulder")
    for n in (["imu4", "imu2", "imu0", "imu5", "imu3"] if has_freeflyer else ["imu4", "imu2", "imu5", "imu3"]):
        add_sensor(m, "ImuSensor", n, frame_name=n)
    return m


def imu_frames(has_freeflyer: bool) -> List[str]:
    return (["imu0"] if has_freeflyer else []) + ["imu2", "imu3", "imu4", "imu5"]


def deformation_test_models() -> List[CompiledModel]:
    """The topologies the GPU tests of the block run the engine with."""
    return [flex_arm(False), flex_arm(True)]
