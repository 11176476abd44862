#!/usr/bin/env python3
"""Per-kernel ISA statistics of the exact-shape builds: compiles rware_static.hip for the given table groups to assembly
(device only) and prints, per rw::rware_step_kernel instantiation, the instruction count, VGPRs, SGPRs, scratch and LDS.
Usage: isa_stats.py OUTDIR [group ...]   (default groups: 0).  Used to check that a refactor leaves the BASELINE builds'
instruction streams alone: diff two outputs.
The group `capi` is rware_capi.hip instead — every kernel of that translation unit (the view, seed and store-floor kernels of the engine
core and the learner-side kernels of rware_snapshot.h, rware_minibatch.h, rware_global_state.h), under its demangled name.
RWARE_ISA_CSRC=<dir>: compile that csrc directory instead of this tree's (a `git worktree` of another commit);
RWARE_ISA_JSON=<file>: also write {"hipcc": <hipcc --version>, "kernels": {"g<group> <instantiation>": {inst, ophash, vgpr, sgpr, lds,
scratch}}} — what tests/golden/isa/static_parent.json holds (tests/test_packed_obs.py compares the tree's builds against it)."""
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.environ.get("RWARE_ISA_CSRC") or os.path.join(ROOT, "robotic-warehouse_amd", "csrc")


def main():
    out = sys.argv[1]
    groups = [g if g == "capi" else int(g) for g in sys.argv[2:]] or [0]
    os.makedirs(out, exist_ok=True)
    record = {}
    procs = []
    for g in groups:
        s = os.path.join(out, "capi.s" if g == "capi" else f"static_g{g}.s")
        unit = ["rware_capi.hip"] if g == "capi" else [f"-DRW_STATIC_GROUP={g}", "rware_static.hip"]
        procs.append((g, s, subprocess.Popen(
            ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-mllvm",
             "-amdgpu-kernarg-preload-count=16", "--cuda-device-only", "-S", "-o", s] + unit[:-1] + [os.path.join(CSRC, unit[-1])])))
    for g, s, p in procs:
        assert p.wait() == 0
        lines = open(s).read().splitlines()
        if g == "capi":  # every kernel of the unit: the symbols that have a kernel descriptor
            kernels = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
            starts = [i for i, l in enumerate(lines) if l.split(":")[0] in kernels and re.match(r"^\S+:\s*(;.*)?$", l)]
        else:
            starts = [i for i, l in enumerate(lines) if re.match(r"^_ZN2rw17rware_step_kernel.*:\s*(;.*)?$", l)]
        for a, b in zip(starts, starts[1:] + [len(lines)]):
            body = lines[a:b]
            name = subprocess.run(["c++filt", lines[a].split(":")[0]], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"^void rw::rware_step_kernel", "", name).split("(")[0]
            ops = [l.split()[0] for l in body if re.match(r"^\s+[a-z_][a-z0-9_]*(\s|$)", l) and not l.strip().startswith((".", ";"))]
            n_inst = len(ops)
            oph = hashlib.sha1(" ".join(ops).encode()).hexdigest()[:10]
            def meta(key):
                for l in body:
                    m = re.match(rf"^; {key}: (\d+)", l)
                    if m:
                        return int(m.group(1))
                return -1
            record[f"g{g} {name}"] = {"inst": n_inst, "ophash": oph, "vgpr": meta("NumVgprs"), "sgpr": meta("TotalNumSgprs"),
                                      "lds": meta("LDSByteSize"), "scratch": meta("ScratchSize")}
            lds = f" lds {meta('LDSByteSize')}" if g == "capi" else ""
            print(f"g{g} {name}: inst {n_inst} vgpr {meta('NumVgprs')} sgpr {meta('NumSgprs')} total_sgpr {meta('TotalNumSgprs')} scratch {meta('ScratchSize')}{lds} occ {meta('Occupancy')} ophash {oph}")
    if os.environ.get("RWARE_ISA_JSON"):
        ver = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
        ver = "\n".join(l for l in ver.splitlines() if "version" in l)  # (the version lines only: no install paths)
        with open(os.environ["RWARE_ISA_JSON"], "w") as f:
            json.dump({"hipcc": ver, "groups": groups, "kernels": record}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
