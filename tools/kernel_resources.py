#!/usr/bin/env python
"""Print the register / scratch / LDS footprint of the kernels in a built topology library
(llvm-objdump --offloading + llvm-readelf --notes on the gfx950 code objects).
    python tools/kernel_resources.py [--match SUBSTRING ...] LIBRARY ...
Without `--match` the physics kernels (`k_quad`, `k_qcon`, `k_constrained`, `k_batch`) are printed; the observer blocks are
`--match k_mahony --match k_attitude_init --match k_body_observer --match k_deformation_estimator`."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def resources(lib: str):
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        link = os.path.join(tmp, os.path.basename(lib))
        os.symlink(os.path.abspath(lib), link)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", link], cwd=tmp, capture_output=True)
        for co in sorted(glob.glob(os.path.join(tmp, "*gfx950*"))):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                get = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]  # noqa: E731
                name = subprocess.run(["c++filt", get("name")], capture_output=True, text=True).stdout.strip()
                out.append({"kernel": re.sub(r"\(.*", "", name), "vgpr": get("vgpr_count"), "agpr": blk.split()[0],
                            "sgpr": get("sgpr_count"), "vgpr_spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
                            "scratch_B": get("private_segment_fixed_size"), "lds_B": get("group_segment_fixed_size")})
    return out


if __name__ == "__main__":
    args, match = sys.argv[1:], []
    while "--match" in args:
        i = args.index("--match")
        match.append(args[i + 1])
        del args[i:i + 2]
    match = match or ["k_quad", "k_qcon", "k_constrained", "k_batch"]
    for lib in args:
        print(lib)
        for r in resources(lib):
            if any(k in r["kernel"] for k in match):
                print("  ", r)
