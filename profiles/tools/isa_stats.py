#!/usr/bin/env python3
"""Per-kernel ISA statistics of the exact-shape builds: compiles rware_static.hip for the given table groups to assembly
(device only) and prints, per rw::rware_step_kernel instantiation, the instruction count, VGPRs, SGPRs, scratch and LDS.
Usage: isa_stats.py OUTDIR [group ...]   (default groups: 0).  Used to check that a refactor leaves the BASELINE builds'
instruction streams alone: diff two outputs.
The group `capi` is rware_capi.hip instead — every kernel of that translation unit (the view, seed and store-floor kernels of the engine
core and the learner-side kernels of rware_snapshot.h, rware_minibatch.h, rware_global_state.h), under its demangled name.
RWARE_ISA_CSRC=<dir>: compile that csrc directory instead of this tree's (a `git worktree` of another commit);
RWARE_ISA_JSON=<file>: also write {"hipcc": <hipcc --version>, "kernels": {"g<group> <instantiation>": {inst, ophash, vgpr, sgpr, lds,
scratch}}} — what tests/golden/isa/static_parent.json holds.
The two steps are functions the tests load this file for (tests/test_packed_obs.py, test_image_u8.py and test_capi_symbols.py): listings()
compiles groups to assembly, fingerprints() reads the per-kernel figures out of one listing; hipcc_version() is the "hipcc" of the JSON."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.environ.get("RWARE_ISA_CSRC") or os.path.join(ROOT, "robotic-warehouse_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIGURES = {"vgpr": "NumVgprs", "sgpr": "TotalNumSgprs", "lds": "LDSByteSize", "scratch": "ScratchSize"}


def hipcc_version():
    """The version lines of `hipcc --version` (no install paths)."""
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    return "\n".join(l for l in out.splitlines() if "version" in l)


def listings(out_dir, groups, csrc=CSRC):
    """Compiles the table groups `groups` of rware_static.hip (`capi`: rware_capi.hip), side by side, to gfx950 assembly under `out_dir`
    -> {group: path of its listing}."""
    os.makedirs(out_dir, exist_ok=True)
    procs = {}
    for g in groups:
        s = os.path.join(out_dir, "capi.s" if g == "capi" else f"static_g{g}.s")
        unit = ["rware_capi.hip"] if g == "capi" else [f"-DRW_STATIC_GROUP={g}", "rware_static.hip"]
        procs[g] = s, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-mllvm", "-amdgpu-kernarg-preload-count=16",
             "--cuda-device-only", "-S", "-o", s] + unit[:-1] + [os.path.join(csrc, unit[-1])], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for g, (s, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err.decode()[-2000:]
    return {g: s for g, (s, _) in procs.items()}


def fingerprints(listing, every_kernel=False, figures=FIGURES):
    """{instantiation: {inst, ophash, vgpr, sgpr, lds, scratch}} per rw::rware_step_kernel of an assembly listing (`every_kernel`: per
    symbol with a kernel descriptor, under its demangled name): the instruction count, a hash of the opcode sequence and `figures` (key ->
    the name of a metadata comment of the kernel; -1: not given)."""
    lines = listing.splitlines()
    if every_kernel:
        kernels = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
        starts = [i for i, l in enumerate(lines) if l.split(":")[0] in kernels and re.match(r"^\S+:\s*(;.*)?$", l)]
    else:
        starts = [i for i, l in enumerate(lines) if re.match(r"^_ZN2rw17rware_step_kernel.*:\s*(;.*)?$", l)]
    out = {}
    for a, b in zip(starts, starts[1:] + [len(lines)]):
        body = lines[a:b]
        name = subprocess.run(["c++filt", lines[a].split(":")[0]], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^void rw::rware_step_kernel", "", name).split("(")[0]
        ops = [l.split()[0] for l in body if re.match(r"^\s+[a-z_][a-z0-9_]*(\s|$)", l) and not l.strip().startswith((".", ";"))]

        def meta(key):
            return next((int(m.group(1)) for l in body for m in [re.match(rf"^; {key}: (\d+)", l)] if m), -1)
        out[name] = dict({"inst": len(ops), "ophash": hashlib.sha1(" ".join(ops).encode()).hexdigest()[:10]}, **{k: meta(v) for k, v in figures.items()})
    return out


def main():
    groups = [g if g == "capi" else int(g) for g in sys.argv[2:]] or [0]
    record = {}
    for g, s in listings(sys.argv[1], groups).items():
        for name, f in fingerprints(open(s).read(), g == "capi", dict(FIGURES, user_sgpr="NumSgprs", occ="Occupancy")).items():
            record[f"g{g} {name}"] = {k: f[k] for k in ("inst", "ophash", *FIGURES)}
            lds = f" lds {f['lds']}" if g == "capi" else ""
            print(f"g{g} {name}: inst {f['inst']} vgpr {f['vgpr']} sgpr {f['user_sgpr']} total_sgpr {f['sgpr']} scratch {f['scratch']}{lds} occ {f['occ']} ophash {f['ophash']}")
    if os.environ.get("RWARE_ISA_JSON"):
        with open(os.environ["RWARE_ISA_JSON"], "w") as f:
            json.dump({"hipcc": hipcc_version(), "groups": groups, "kernels": record}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
