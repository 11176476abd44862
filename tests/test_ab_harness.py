"""profiles/tools/ab.py, the one A/B harness: its leg runner (child processes, exactly as the tool starts them — on the CPU against the
host-thread emulation library), its orchestrator (a failing leg ends the run), its acceptance rule on constructed lists, and that every
experiment it carries resolves without a device.  No test here asserts a time against a bound."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

import rware_amd
from rware_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = os.path.join(ROOT, "profiles", "tools", "ab.py")
SMALL4 = "rware-small-4ag-v1"
_spec = importlib.util.spec_from_file_location("ab_harness", AB)
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)


@pytest.fixture(scope="module")
def emu():
    from engine_backend import build_emu
    return build_emu()


def run_leg(**spec):
    p = subprocess.run([sys.executable, AB, "--leg", json.dumps(spec)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def run_tool(*argv):
    return subprocess.run([sys.executable, AB] + [str(a) for a in argv], capture_output=True, text=True, timeout=600)


def report_legs(text):
    """{configuration: {leg: identity columns}} of a report: the leg lines are the indented ones that carry them."""
    out, config = {}, None
    for line in text.splitlines():
        if line and not line.startswith((" ", "#")):
            config = line
        elif "   build_kind " in line:
            out.setdefault(config, {})[line.split()[0]] = line.split("   build_kind ")[1]
    return out


# rware-small-4ag-v1 x 32 envs (two 16-env workgroups), a tape of 4 rows, 2 warm-up + 4 timed steps
CPU_LEGS = {
    "step": dict(mode="step", options={}),
    "step, action_mask": dict(mode="step", options={"action_mask": True}),
    "step, time_limit_truncates": dict(mode="step", options={"time_limit_truncates": True}),
    "rollout, K = 4": dict(mode="rollout", options={}),
    "step+unpack, obs_packed": dict(mode="step+unpack", options={"obs_packed": True}),
    "IMAGE, obs_image_u8": dict(mode="step", observation_type=2, options={"obs_image_u8": True}),
}


@pytest.mark.parametrize("case", list(CPU_LEGS))
def test_leg_on_the_emulation_library(emu, case):
    leg = CPU_LEGS[case]
    r = run_leg(lib=emu, env_id=SMALL4, envs=32, steps=4, warmup=2, tape=4, **leg)
    assert set(r) == {"us_per_step", "steps", "build_kind", "jit", "E", "nt", "stats", "obs_packed", "bytes", "abi", "env0_steps"}
    assert r["us_per_step"] > 0 and r["steps"] == 4 and r["abi"] == _capi.RW_ABI_VERSION and r["bytes"] > 0
    if leg["mode"] == "rollout":
        assert r["env0_steps"] == 4 + 4        # one warm-up launch of K = 4 fused steps, one timed
    else:
        assert r["env0_steps"] == 2 + 4
    opts = leg["options"]
    assert r["stats"] == (4 if opts.get("action_mask") else 0) | (8 if opts.get("time_limit_truncates") else 0)   # rw_info.stats, a bit set
    assert r["obs_packed"] == (1 if opts.get("obs_packed") else 2 if opts.get("obs_image_u8") else 0)


def test_a_leg_names_the_symbol_its_mode_lacks(tmp_path):
    """A parent commit's library may be older than the description: the symbol is named, nothing is called."""
    src = tmp_path / "old.c"
    src.write_text("int rw_abi_version(void) { return 4; }\n")
    lib = tmp_path / "libold.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(src)])
    p = run_tool("--leg", json.dumps(dict(lib=str(lib), env_id=SMALL4, envs=32, steps=4, warmup=2, mode="step", options={})))
    assert p.returncode != 0 and "rw_step_tape_device_timed" in p.stderr and "lacks" in p.stderr


def test_a_failing_leg_ends_the_run(emu, tmp_path):
    tiny = ["--envs", 32, "--steps", 4, "--warmup", 2, "--tape", 4, "--reps", 2, "--only", "x 16384"]
    p = run_tool("baseline", "--parent-lib", emu, "--own-lib", tmp_path / "no_such_library.so", *tiny)
    started = [l for l in p.stdout.splitlines() if l.startswith("rep ") and " leg " in l]
    assert p.returncode != 0 and "failed" in p.stderr
    assert len(started) == 1 and " leg a:" in started[0]      # the parent's leg ran, this tree's failed, no third was started


def test_orchestrator_reports_one_line_per_leg(emu, tmp_path):
    out = tmp_path / "report.txt"
    p = run_tool("baseline", "--parent-lib", emu, "--own-lib", emu, "--envs", 32, "--steps", 4, "--warmup", 2, "--tape", 4, "--reps", 1,
                 "--only", "small-4ag x 262144", "--out", out)
    assert p.returncode == 0, p.stdout + p.stderr
    assert len([l for l in p.stdout.splitlines() if l.startswith("rep ")]) == 3
    legs = report_legs(out.read_text())
    assert list(legs) == ["small-4ag x 262144"] and list(legs["small-4ag x 262144"]) == ["a", "b", "a2"]
    assert len(set(legs["small-4ag x 262144"].values())) == 1
    assert "b / a + a2: " in out.read_text() and "the spread" in out.read_text()


def test_verdict_on_constructed_runs():
    v = ab.verdict
    assert v([10.1, 10.3, 10.2], [10.0, 10.4, 10.2, 9.9])["word"] == "inside"         # ratio 1.0099 in 0.952 .. 1.051
    assert v([10.7, 10.8, 10.9], [10.0, 10.4, 10.2, 9.9])["word"] == "OUTSIDE"        # above: 1.069
    assert v([9.3, 9.4, 9.5], [10.0, 10.4, 10.2, 9.9])["word"] == "OUTSIDE"           # below: 0.931
    r = v([10.1, 10.3, 10.2], [10.0, 10.4, 10.2, 9.9])
    assert r["ratio"] == pytest.approx(10.2 / 10.1) and r["lo"] == pytest.approx(9.9 / 10.4) and r["hi"] == pytest.approx(10.4 / 9.9)
    assert v([5.0, 5.0], [5.0, 5.0, 5.0])["word"] == "inside"                         # identical parent runs: only ratio 1 ...
    assert v([5.0, 5.001], [5.0, 5.0, 5.0])["word"] == "OUTSIDE" and v([4.999, 5.0], [5.0, 5.0])["word"] == "OUTSIDE"   # ... is inside
    one = v([5.0, 5.0], [5.0])
    assert one["word"] == "no spread" and "inside" not in one["text"] and one["ratio"] == 1.0
    assert "(max - min) / median" in r["text"]


def test_every_experiment_resolves_without_a_device():
    assert set(ab.EXPERIMENTS) == {"baseline", "action_mask", "time_limit", "packed_obs", "image_u8", "reset_device", "global_image"}
    for name, exp in ab.EXPERIMENTS.items():
        assert exp["reps"] >= 1 and exp["configs"] and exp["compare"], name
        for conf in list(exp["configs"].values()) + [spec for _, spec in exp.get("extras", ())]:
            rware_amd.env_kwargs(conf["env_id"])                                      # registered (KeyError otherwise)
            assert conf.get("mode", "step") in ab.NEEDS and conf.get("fn", "step") in ab.LEG_FUNCTIONS
        for leg in exp["legs"].values():
            assert leg["lib"] in ("parent", "own") and (leg["mode"] is None or leg["mode"] in ab.NEEDS)
            assert _capi.stream_flags(**leg["options"]) >= 0
            assert all(v is True for v in leg["options"].values()), "options are given by keyword, never as numbers"
        for own, parents in exp["compare"]:
            assert exp["legs"][own]["lib"] == "own" and parents and all(exp["legs"][p]["lib"] == "parent" for p in parents), name
    base = ab.EXPERIMENTS["baseline"]
    assert [(l["lib"], l["options"]) for l in base["legs"].values()] == [("parent", {}), ("own", {}), ("parent", {})]
    assert [(c["envs"], c["mode"]) for c in base["configs"].values()] == [(16384, "step"), (262144, "step"), (16384, "rollout")]
    for mode, names in ab.NEEDS.items():
        assert set(names) <= set(_capi.PROTOTYPES), mode


# -- on the GPU: the harness, not a kernel, is under test, so the shapes are tiny --------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode, options", [("step", {}), ("rollout", {}), ("step+unpack", {"obs_packed": True})])
def test_gpu_leg_per_mode(mode, options):
    r = run_leg(lib=_capi.DEFAULT_LIBRARY, env_id=SMALL4, envs=64, steps=8, warmup=8, tape=8, mode=mode, options=options)
    assert r["steps"] == 8 and r["env0_steps"] == 16 and r["obs_packed"] == (1 if options else 0) and r["us_per_step"] > 0


@pytest.mark.gpu
def test_gpu_baseline_of_the_tree_against_itself(tmp_path):
    out = tmp_path / "report.txt"
    p = run_tool("baseline", "--parent-lib", _capi.DEFAULT_LIBRARY, "--reps", 1, "--only", "x 16384", "--steps", 64, "--out", out)
    assert p.returncode == 0, p.stdout + p.stderr
    legs = report_legs(out.read_text())
    assert list(legs) == ["small-4ag x 16384", "rollout-64: small-4ag x 16384"]
    for config, rows in legs.items():
        assert list(rows) == ["a", "b", "a2"], config                                 # one line per leg
        assert rows["a"] == rows["b"] == rows["a2"], config                           # parent and own: the same engine, the same launches
    assert out.read_text().count("the spread") == 2


def test_the_further_experiments_resolve_without_a_device():
    spec = importlib.util.spec_from_file_location("ab_harness_more", os.path.join(ROOT, "profiles", "tools", "ab.py"))
    ab = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ab)
    assert set(ab.MORE_EXPERIMENTS) == {"restore_indexed"} and not set(ab.MORE_EXPERIMENTS) & set(ab.EXPERIMENTS)
    for name, exp in ab.MORE_EXPERIMENTS.items():
        assert exp["reps"] >= 1 and exp["configs"] and exp["compare"], name
        for conf in list(exp["configs"].values()) + [s for _, s in exp.get("extras", ())]:
            rware_amd.env_kwargs(conf["env_id"])                                      # registered (KeyError otherwise)
            assert conf.get("mode", "step") in ab.NEEDS and conf.get("fn", "step") in ab.LEG_FUNCTIONS
        for leg in exp["legs"].values():
            assert leg["lib"] in ("parent", "own") and (leg["mode"] is None or leg["mode"] in ab.NEEDS)
            assert _capi.stream_flags(**leg["options"]) >= 0
            assert all(v is True for v in leg["options"].values()), "options are given by keyword, never as numbers"
        for own, parents in exp["compare"]:
            assert exp["legs"][own]["lib"] == "own" and parents and all(exp["legs"][p]["lib"] == "parent" for p in parents), name
    exp = ab.MORE_EXPERIMENTS["restore_indexed"]
    assert exp["configs"] is ab.THREE and exp["legs"] is ab.PARENT_OWN_PARENT       # the per-step legs are `baseline`'s
    assert [(s["fn"], s["envs"]) for _, s in exp["extras"]] == [("restore", 16384), ("restore", 262144), ("restore", 16384)]
