"""Cost of moving an emitter: prt_scene_refit_device with prt_scene_set_dynamic_lights on (the light tree, its records and
its O(1) tables follow on the device) against prt_scene_update_vertices (the only way to move a light without the switch:
host positions, every table re-sent, the light tables built on the host), on the same motion.  One GPU.

  python tools/light_update_timing.py [--scenes veach-mis,cornell,sphere100k] [--runs 20] [--out profiles/light_update_timing.json]

Every scene is one child process under its own `timeout`; the first child that fails ends the run, and what it had printed
(one JSON line per figure, tools/timing_common.py) is still written.  Per scene the child alternates between two vertex
sets (the start, and every emitter vertex displaced by timing_common.wobble, 1 % of the emitters' extent) and records
medians over --runs calls after a warm-up, wall and hipEvent milliseconds, of
  refit_device_lights   refit_device with the switch on and the emitters moving, with the medians of its
                        gather_ms / host_tree_ms / tables_ms split (PrtLightUpdateInfo)
  refit_device_still    refit_device with the switch on and the same positions as resident (emitters still; the read-back
                        carries the emitters' vertices) and with the switch off (the call as it was before the switch existed)
  update_vertices       the yardstick, on the same motion
There is no pass threshold: the numbers are quoted in DESIGN.md §7 and the README.
"""
import argparse
import functools
import os
import statistics
import sys

import timing_common as tc

SCENES = ("veach-mis", "cornell", "sphere100k")
GROUPS = {"update": "update"}
CAMERA = {"veach-mis": dict(width=256, height=144), "cornell": dict(width=256, height=256)}


def sphere_in_a_box(s):
    """A synthetic emissive icosphere of 81,920 triangles (subdivision 6: the nearest icosphere to 100k) in a closed box."""
    from pooraytracer_amd import _abi
    b = s._Builder("sphere100k")
    white = b.material(s.Material("white", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    light = b.material(s.Material("Light", _abi.MAT_DIFFUSE_LIGHT, emission=(8.0, 8.0, 8.0)))
    b.mesh("box", white, *s.box((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)))
    v, uv, n = s.icosphere(6, radius=0.6, center=(0.0, 0.3, 0.0))
    b.mesh("lamp", light, v, uv, n)
    return b.build(s.Camera(256, 256, 60.0, eye=(0.0, 0.0, 1.9), look_at=(0.0, 0.0, 0.0)))


def child(name, runs):
    import numpy as np
    import torch
    from pooraytracer_amd import api, build, scenes
    build.build()
    data = sphere_in_a_box(scenes) if name == "sphere100k" else tc.load(name, **CAMERA[name])[0]
    mask = tc.emitter_mask(data)  # here the emitters move and the rest stays
    sets = [tc.wobble(data.vertices, mask), data.vertices.copy()]
    d_sets = [torch.from_numpy(v).cuda() for v in sets]
    d_n = torch.from_numpy(np.ascontiguousarray(data.normals)).cuda()
    sc = api.Scene(data).upload(0)
    sc.dynamic_lights = True
    tc.emit(n_tris=data.n_tris, emitter_tris=int(mask.sum()), runs=runs)

    update = functools.partial(tc.emit_timed, "light_update_timing " + name, "update", n=runs)
    split = []  # PrtLightUpdateInfo behind every counted call
    fast = update("refit_device_lights", lambda i: sc.refit_device(d_sets[i % 2].data_ptr(), d_n.data_ptr()),
                  after=lambda: split.append(sc.light_update_info()),
                  more=lambda: {k: statistics.median(e[k] for e in split) for k in ("gather_ms", "host_tree_ms", "tables_ms")})
    lu = sc.light_update_info()
    assert lu["updates"] == runs + 2 and lu["tables_dropped"] == 0, lu
    tc.emit(tables={k: lu[k] for k in ("n_tables", "table_words", "relaid")})
    resident = d_sets[(runs + 1) % 2]
    update("refit_device_still", lambda i: sc.refit_device(resident.data_ptr(), d_n.data_ptr()))
    assert sc.light_update_info()["updates"] == runs + 2
    sc.dynamic_lights = False
    update("refit_device_still_switch_off", lambda i: sc.refit_device(resident.data_ptr(), d_n.data_ptr()))
    slow = update("update_vertices", lambda i: sc.update_vertices(sets[i % 2], normals=data.normals), warm=1)
    tc.emit(update="speedup_over_update_vertices_wall", result=slow["wall_ms"] / fast["wall_ms"])
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    tc.common_args(ap, launches=False, runs=20, out=os.path.join(tc.ROOT, "profiles", "light_update_timing.json"), worker=True)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.runs)
    names = tc.scene_names(ap, args.scenes, SCENES)
    return tc.write_result(tc.run_children(__file__, names, tc.flags(args, "runs"), {"sphere100k": 420}, GROUPS), args.out)


if __name__ == "__main__":
    sys.exit(main())
