"""Pins of the reference's robot descriptions for tests/test_model_compiler.py, so that the suite needs no copy of the
reference tree: numbers derived from its URDF files, never the files themselves, written to tests/golden/ref_urdf.npz.

    python tools/make_urdf_fixtures.py <reference tree>      (or JIMINY_REFERENCE=<reference tree>)

Entries:
  anymal_model_{signature,inertia,placement_R}   `build_robot` on the reference's anymal.urdf (free-flyer)
  <robot>_{mass,com,inertia}                     `_urdf_composite` of the test module: total mass, centre of mass and
                                                 composite inertia about the root-link origin, walked from the XML alone
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden", "ref_urdf.npz")
URDFS = {
    "anymal": "data/quadrupedal_robots/anymal/anymal.urdf",
    "atlas": "data/bipedal_robots/atlas/atlas.urdf",
}


def main(ref: str, out: str = OUT) -> None:
    sys.path.insert(0, ROOT)
    from jiminy_amd.model import build_robot
    from tests.test_model_compiler import _urdf_composite

    m = build_robot(os.path.join(ref, URDFS["anymal"]), has_freeflyer=True, name="anymal")
    fix = {"anymal_model_signature": np.array(m.topology_signature()),
           "anymal_model_inertia": np.asarray(m.inertia, dtype=np.float64),
           "anymal_model_placement_R": np.asarray(m.placement_R, dtype=np.float64)}
    for name, rel in URDFS.items():
        mass, com, inertia = _urdf_composite(os.path.join(ref, rel))
        fix[f"{name}_mass"] = np.array(mass, dtype=np.float64)
        fix[f"{name}_com"] = np.asarray(com, dtype=np.float64)
        fix[f"{name}_inertia"] = np.asarray(inertia, dtype=np.float64)
    np.savez_compressed(out, **fix)
    print(f"wrote {os.path.relpath(out, ROOT)}: {len(fix)} entries")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("JIMINY_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    main(ref)
