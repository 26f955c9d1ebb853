"""CPU tests of tools/timing_common.py, the module the tools/*_timing.py programs share, and of what every such tool must keep:
a `--help` that needs neither torch nor a built library, the refusal of medians of fewer than 10 launches, and one
definition of each shared piece.  The children that run_children starts here are tiny scripts written into tmp_path; they
never touch the GPU or import the package.
"""
import glob
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from pooraytracer_amd import _abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import timing_common as tc  # noqa: E402

NAMES = ("adaptive", "closest_point", "denoise_guided", "denoise", "light_update", "multi_hit", "occlusion", "progressive",
         "ray_color", "rebuild", "refit", "signed_distance", "surface", "winding")
WITH_LAUNCHES = ("closest_point", "multi_hit", "occlusion", "ray_color", "signed_distance", "surface", "winding")


def test_the_fourteen_tools_are_the_tools():
    assert sorted(glob.glob(os.path.join(TOOLS, "*_timing.py"))) == sorted(os.path.join(TOOLS, n + "_timing.py") for n in NAMES)


# ---- stats, interleaved

def test_stats_odd_and_even():
    assert tc.stats([3.0, 1.0, 2.0]) == {"median_ms": 2.0, "min_ms": 1.0, "max_ms": 3.0}
    # an even list: the upper middle element, s[len(s) // 2], not the mean of the two
    assert tc.stats([4.0, 1.0, 3.0, 2.0]) == {"median_ms": 3.0, "min_ms": 1.0, "max_ms": 4.0}
    assert tc.stats([0.123456, 0.2]) == {"median_ms": 0.2, "min_ms": 0.1235, "max_ms": 0.2}
    assert tc.stats([7.0]) == {"median_ms": 7.0, "min_ms": 7.0, "max_ms": 7.0}


def test_interleaved_order_and_counts():
    log = []

    def fake(name):
        def fn():
            log.append(name)
            return {"kernel_ms": float(len(log)), "who": name, "at": len(log)}
        return fn

    names = ["a", "b", "c"]
    ms, last = tc.interleaved([(n, fake(n)) for n in names], launches=4, warmup=2)
    assert log == names * 2 + names * 4  # the warm-up rounds, then exactly `launches` rounds, in list order
    assert list(ms) == names and all(len(v) == 4 for v in ms.values())
    assert ms["a"] == [7.0, 10.0, 13.0, 16.0] and ms["c"] == [9.0, 12.0, 15.0, 18.0]  # nothing of the warm-up is counted
    assert {n: last[n]["at"] for n in names} == {"a": 16, "b": 17, "c": 18}


# ---- the motion

def three_meshes():
    """A box, an emitting quad and a coarse ball: the emitter is the middle mesh, so its triangles are an inner slice."""
    b = scenes._Builder("three")
    white = b.material(scenes.Material("white", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    light = b.material(scenes.Material("Light", _abi.MAT_DIFFUSE_LIGHT, emission=(8.0, 8.0, 8.0)))
    b.mesh("box", white, *scenes.box((-2.0, -1.0, -1.5), (2.0, 1.0, 1.5)))
    b.mesh("lamp", light, *scenes.quad((-0.25, 0.99, -0.25), (0.25, 0.99, -0.25), (0.25, 0.99, 0.25), (-0.25, 0.99, 0.25)))
    b.mesh("ball", white, *scenes.icosphere(1, radius=0.4, center=(0.2, -0.5, 0.1)))
    return b.build(scenes.Camera(32, 32, 60.0, eye=(0.0, 0.0, 1.4), look_at=(0.0, 0.0, 0.0)))


def test_emitter_mask_and_wobble():
    data = three_meshes()
    first = np.asarray(data.mesh_first_tri)
    assert len(data.mesh_material) == 3
    emit = tc.emitter_mask(data)
    want = np.zeros(data.n_tris, dtype=bool)
    want[first[1]:first[2]] = True
    assert np.array_equal(emit, want) and 0 < emit.sum() < data.n_tris
    for mask, amount in ((~emit, 0.01), (emit, 0.01), (~emit, 0.5)):
        got = tc.wobble(data.vertices, mask, amount) if amount != 0.01 else tc.wobble(data.vertices, mask)
        # the formula spelt independently: x + a ext sin(7 / ext (y, z, x) + phase), ext = the moved points' largest extent
        # (whole-array sines on both sides: a vectorised sine need not round like the scalar one)
        idx = np.flatnonzero(mask)
        x = np.stack([data.vertices[t] for t in idx])
        ext = float(max(np.ptp(x[:, :, k]) for k in range(3)))
        yzx = np.roll(x, -1, axis=2)
        exp = data.vertices.copy()
        exp[idx] = x + (amount * ext) * np.sin((7.0 / ext) * yzx + np.array([[[0.3, 1.1, 2.3]]]))
        assert got.dtype == np.float64 and got.tobytes() == exp.tobytes()
        assert np.array_equal(got[~mask], data.vertices[~mask])  # masked-out triangles are untouched
        assert (got[mask] != data.vertices[mask]).any()
        assert got is not data.vertices
    assert np.array_equal(tc.wobble(data.vertices, ~emit, amount=0), data.vertices)  # amount 0: the identity


# ---- the protocol

def test_collect_groups_header_and_junk():
    lines = [
        json.dumps({"n_tris": 12, "launches": 11}),
        "Loading library ...",
        json.dumps({"class": "surface", "result": {"x": 1}}),
        "{not json",
        "17",
        json.dumps({"batch": "s0", "variant": "f64", "result": {"r": 1}}),
        json.dumps({"batch": "s0", "variant": "f32", "result": {"r": 2}}),
        json.dumps({"batch": "miss", "variant": "f64", "result": {"r": 3}}),
        json.dumps({"switch": "refit_device", "result": {"w": 4}}),
        json.dumps({"class": "box", "result": {"x": 2}}),
        json.dumps({"launches": 12, "decay": [1, 2]}),
        "",
    ]
    got = tc.collect("\n".join(lines), {"class": "classes", "switch": "switch", "batch": ("batches", "variant")})
    assert got == {"n_tris": 12, "launches": 12, "decay": [1, 2],
                   "classes": {"surface": {"x": 1}, "box": {"x": 2}}, "switch": {"refit_device": {"w": 4}},
                   "batches": {"s0": {"f64": {"r": 1}, "f32": {"r": 2}}, "miss": {"f64": {"r": 3}}}}
    # a group with no record is there and empty, and a key of no group is header
    assert tc.collect(json.dumps({"variant": "f64", "result": 5}), {"class": "classes"}) == {"classes": {}, "variant": "f64", "result": 5}
    assert tc.collect("", {"variant": "variants"}) == {"variants": {}}


def test_emit_is_one_json_line(capsys):
    tc.emit("for the eye", **{"class": "near"}, result={"a": 1.5})
    tc.emit(n_tris=3)
    cap = capsys.readouterr()
    assert [json.loads(ln) for ln in cap.out.splitlines()] == [{"class": "near", "result": {"a": 1.5}}, {"n_tris": 3}]
    assert cap.err == "for the eye\n"


CHILD = """
import argparse, json, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--child")
ap.add_argument("--tag")
a = ap.parse_args()
open(a.child + ".ran", "w").write(a.tag)
print(json.dumps({"scene_name": a.child, "tag": a.tag}), flush=True)
print("chatter that is no record", flush=True)
print(json.dumps({"class": "first", "result": {"v": 1}}), flush=True)
print(json.dumps({"class": "second", "result": {"v": 2}}), flush=True)
BEHAVIOUR
print(json.dumps({"class": "third", "result": {"v": 3}}), flush=True)
"""
GROUPS = {"class": "classes"}


def fake_child(tmp_path, behaviour):
    script = tmp_path / "fake_timing.py"
    script.write_text(textwrap.dedent(CHILD).replace("BEHAVIOUR", behaviour))
    return str(script)


def test_run_children_all_succeed(tmp_path):
    script = fake_child(tmp_path, "pass")
    out = tc.run_children(script, ["a", "b", "c"], ["--tag", "t1"], 30, GROUPS, tree=str(tmp_path))
    entry = {"tag": "t1", "classes": {"first": {"v": 1}, "second": {"v": 2}, "third": {"v": 3}}}
    assert out == {"scenes": {n: dict(entry, scene_name=n) for n in "abc"}}
    assert list(out["scenes"]) == ["a", "b", "c"]
    assert all((tmp_path / (n + ".ran")).read_text() == "t1" for n in "abc")  # every child ran in the tree it was given


def test_run_children_stops_at_the_first_failure_and_keeps_its_records(tmp_path):
    script = fake_child(tmp_path, 'if a.child == "b": sys.exit(139)')
    out = tc.run_children(script, ["a", "b", "c"], ["--tag", "t2"], 30, GROUPS, tree=str(tmp_path))
    assert out["failed"] == {"scene": "b", "returncode": 139}
    assert list(out["scenes"]) == ["a", "b"]
    assert out["scenes"]["a"]["classes"] == {"first": {"v": 1}, "second": {"v": 2}, "third": {"v": 3}}
    assert out["scenes"]["b"] == {"scene_name": "b", "tag": "t2", "classes": {"first": {"v": 1}, "second": {"v": 2}}}
    assert (tmp_path / "b.ran").exists() and not (tmp_path / "c.ran").exists()  # nothing was started after the failure


def test_run_children_time_limit_ends_the_run(tmp_path):
    script = fake_child(tmp_path, 'if a.child == "a": time.sleep(60)')
    out = tc.run_children(script, ["a", "b"], ["--tag", "t3"], 1, GROUPS, tree=str(tmp_path))
    assert out["failed"] == {"scene": "a", "returncode": 124}
    assert out["scenes"] == {"a": {"scene_name": "a", "tag": "t3", "classes": {"first": {"v": 1}, "second": {"v": 2}}}}
    assert not (tmp_path / "b.ran").exists()


def test_run_children_then_hook_may_fail_the_run(tmp_path):
    script = fake_child(tmp_path, "pass")
    seen = []

    def then(name, entry):
        seen.append((name, entry["tag"]))
        return {"scene": name, "returncode": 7} if name == "b" else None

    out = tc.run_children(script, ["a", "b", "c"], ["--tag", "t4"], 30, GROUPS, tree=str(tmp_path), then=then)
    assert seen == [("a", "t4"), ("b", "t4")] and out["failed"] == {"scene": "b", "returncode": 7}
    assert not (tmp_path / "c.ran").exists()


def test_scene_table():
    for name in ("cornell-box", "bathroom2", "veach-mis", "soup1m", "soup8m", "cornell"):
        factory, kw, device_bvh, limit = tc.scene(name)
        assert callable(getattr(scenes, factory)) and isinstance(kw, dict) and isinstance(device_bvh, bool) and limit > 0
    assert tc.scene("soup8m")[3] == 1100 and tc.scene("cornell-box")[3] == 900  # the larger of the limits the tools had
    data, device_bvh = tc.load("cornell", ball_subdiv=1, width=16)
    assert (data.camera.width, data.camera.height, device_bvh) == (16, 512, False)


def test_write_result_makes_the_directory(tmp_path, capsys):
    path = tmp_path / "not" / "there" / "yet.json"
    assert tc.write_result({"scenes": {}, "x": 1}, str(path)) == 0
    assert path.read_text() == '{"scenes": {}, "x": 1}\n' == capsys.readouterr().out
    assert tc.write_result({"failed": {"scene": "a", "returncode": 1}}, "") == 1


# ---- every tool

def run_tool(name, *argv):
    """The tool as `python tools/<name>_timing.py argv`, through a wrapper that reports whether torch was imported."""
    tool = os.path.join(TOOLS, name + "_timing.py")
    wrapper = ("import runpy, sys\n"
               "sys.argv = sys.argv[1:]\n"
               "sys.path.insert(0, %r)\n"
               "try:\n"
               "    runpy.run_path(sys.argv[0], run_name='__main__')\n"
               "    code = 0\n"
               "except SystemExit as e:\n"
               "    code = e.code or 0\n"
               "print('TORCH' if 'torch' in sys.modules or 'numpy' in sys.modules else 'LEAN')\n"
               "sys.exit(code)\n") % TOOLS
    env = {k: v for k, v in os.environ.items() if k not in ("CUDA_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES")}
    return subprocess.run([sys.executable, "-c", wrapper, tool, *argv], capture_output=True, text=True, cwd=ROOT, env=env)


@pytest.mark.parametrize("name", NAMES)
def test_tool_help_needs_no_torch(name):
    r = run_tool(name, "--help")
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("usage: ") and r.stdout.rstrip().endswith("LEAN"), r.stdout[-200:]
    flags = r.stdout
    assert "--out" in flags or name == "progressive"
    if name in WITH_LAUNCHES:
        assert "--launches" in flags and "--warmup" in flags and "--child" in flags
    if name in ("refit", "rebuild", "light_update"):
        assert "--worker" in flags and "--runs" in flags


@pytest.mark.parametrize("name", WITH_LAUNCHES)
def test_tool_refuses_a_median_of_nine(name):
    r = run_tool(name, "--launches", "9")
    assert r.returncode == 2
    assert r.stderr.rstrip().endswith("error: --launches: the median of at least 10 launches"), r.stderr
    assert r.stdout.rstrip().endswith("LEAN")


# ---- one definition of each shared piece

def sources():
    paths = sorted(glob.glob(os.path.join(TOOLS, "*_timing.py"))) + [os.path.join(TOOLS, "timing_common.py")]
    return {os.path.basename(p): open(p).read() for p in paths}


@pytest.mark.parametrize("text", ["def stats", "def collect", "np.sin(7.0", "enable_timing=True", "def rel_mse", "def timed_calls"])
def test_defined_once(text):
    where = {name: src.count(text) for name, src in sources().items() if text in src}
    assert where == {"timing_common.py": 1}, where


def test_only_the_shared_module_starts_processes():
    for name, src in sources().items():
        if name != "timing_common.py":
            assert "subprocess" not in src and "Popen" not in src and "os.system" not in src and "os.exec" not in src, name
    assert sources()["timing_common.py"].count("subprocess.run(") == 1 and "Popen" not in sources()["timing_common.py"]
