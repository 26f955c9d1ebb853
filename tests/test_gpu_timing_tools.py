"""GPU tests (-m gpu) of the measuring half of tools/timing_common.py, in-process on the smallest scene that has an emitter
and a non-emitter mesh: the cornell box with its coarsest ball and a 32 x 32 camera.  What the figures mean is the tools'
business; here only that the loops count what they say they count and leave the scene as they found it.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from pooraytracer_amd import api, scenes

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import timing_common as tc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data(gpu):
    return scenes.cornell_box(ball_subdiv=0, width=32, height=32)


def test_timed_calls_counts_and_indices(data, capsys):
    sc = api.Scene(data).upload(0)
    d_v = torch.from_numpy(np.ascontiguousarray(data.vertices)).cuda()
    seen, behind = [], []

    def fn(i):
        seen.append(i)
        sc.refit_device(d_v.data_ptr())

    wall, evt = tc.timed_calls(fn, 4, after=lambda: behind.append(len(seen)))
    capsys.readouterr()
    emitted = tc.emit_timed("test", "update", "refit_device", fn, 2, warm=1, calls=False, more=lambda: {"seen": len(seen)})
    assert json.loads(capsys.readouterr().out) == {"update": "refit_device", "result": emitted}
    assert emitted["seen"] == 9 and "calls" not in emitted and emitted["wall_ms"] > 0
    del seen[6:]
    sc.close()
    assert seen == [0, 1, 2, 3, 4, 5]  # two warm-up calls, then the four that count
    assert behind == [3, 4, 5, 6]  # `after` runs behind each counted call only
    assert len(wall) == 4 and len(evt) == 4 and min(wall) > 0 and min(evt) > 0
    row = tc.summary(wall, evt)
    assert row["calls"] == 4 and row["wall_min_ms"] <= row["wall_ms"] <= row["wall_max_ms"]
    assert "calls" not in tc.summary(wall, evt, calls=False)


def test_switch_blocks_is_fair_and_ends_on_the_start_geometry(data):
    sc = api.Scene(data).upload(0)
    start = np.ascontiguousarray(data.vertices)
    moved = tc.wobble(start, ~tc.emitter_mask(data))
    assert (moved != start).any()
    d_sets = [torch.from_numpy(moved).cuda(), torch.from_numpy(start).cuda()]
    states = []

    def set_state(state):
        states.append(state)
        sc.distance_queries = state == "on"

    res = dict(tc.switch_blocks(sc, start, d_sets, 4, ("off", "on"), set_state))
    assert list(res) == ["refit_device", "rebuild_device"]
    for call, rows in res.items():
        assert list(rows) == ["off", "on"], call
        assert rows["off"]["calls"] == rows["on"]["calls"] >= 4 and rows["off"]["calls"] % 2 == 0, (call, rows)
        assert all(rows[s][k] > 0 for s in rows for k in ("wall_ms", "event_ms", "wall_min_ms")), (call, rows)
    assert states == ["off", "on"] * (len(states) // 2) and sc.distance_queries
    # the resident geometry is the start geometry again
    lo, hi = data.bounds()
    rays = scenes.random_rays(256, lo, hi, seed=5)
    got = sc.trace_closest(rays)
    sc.close()
    fresh = api.Scene(data).upload(0)
    want = fresh.trace_closest(rays)
    fresh.close()
    assert (want["prim"] >= 0).any()
    assert got.tobytes() == want.tobytes()


def test_interleaved_on_two_kernels(data):
    sc = api.Scene(data).upload(0)
    n = 4096
    lo, hi = data.bounds()
    d_r = torch.from_numpy(scenes.random_rays(n, lo, hi, seed=6).view(np.float64).reshape(-1, 8)).cuda()
    d_h = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d_o = torch.zeros(n, dtype=torch.uint8, device="cuda")
    calls = [("closest", tc.launcher(sc, sc.trace_closest_device, d_r.data_ptr(), n, d_h.data_ptr())),
             ("occluded", tc.launcher(sc, sc.trace_occluded_device, d_r.data_ptr(), n, d_o.data_ptr()))]
    ms, last = tc.interleaved(calls, launches=10, warmup=2)
    counted = calls[0][1](count_work=True)
    sc.close()
    assert list(ms) == ["closest", "occluded"]
    assert all(len(v) == 10 and min(v) > 0 for v in ms.values()), ms
    assert all(last[k]["kernel_ms"] == ms[k][-1] for k in ms)
    assert counted["node_fetches"] > 0  # keywords given to a launcher's call reach the method
    st = tc.stats(ms["closest"])
    assert st["min_ms"] <= st["median_ms"] <= st["max_ms"]
