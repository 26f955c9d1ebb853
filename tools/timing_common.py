"""What the tools/*_timing.py programs share: how a figure is taken, and how GPU work is kept in child processes.

Measuring (torch and numpy are imported where they are used, so that `--help` and the driver half need neither):
  stats, interleaved, launcher   medians of kernel_ms (prt_get_counters) of launches that take turns
  timed_calls, summary           wall and hipEvent milliseconds around single calls
  emitter_mask, wobble           the one sinusoidal motion of the geometry-update figures
  switch_blocks                  refit_device / rebuild_device under switch states that alternate in blocks
  rel_mse                        the image error of the accumulator and denoiser tools
The child protocol: a child prints every figure as one JSON line as soon as it has it (`emit`), the parent folds the lines
into one entry per scene (`collect`), so what a failed child had measured is kept.  `run_children` starts one child per
scene under its own `timeout -k 10`, in the tree it measures, and starts nothing more after the first child that fails
(a fault may have left the GPU in a state that the next process would only make worse).  `spawn` is the only place where
a *_timing.py tool starts a process.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("PRT_TIMING_TREE") or ROOT  # the checkout whose package and library a child times
if TREE not in sys.path:
    sys.path.insert(0, TREE)

# name -> (scenes factory, keywords, tree built on the GPU, seconds a child may take)
_SCENES = {
    "cornell-box": ("cornell_box", {}, False, 900),
    "cornell": ("cornell_box", {"width": 512, "height": 512}, False, 240),  # the geometry-update tools' small frame
    "bathroom2": ("bathroom", {}, False, 900),
    "veach-mis": ("veach_mis", {}, False, 240),
    "soup1m": ("triangle_soup", {"n_tris": 1_000_000}, True, 900),
    "soup8m": ("triangle_soup", {"n_tris": 8_000_000}, True, 1100),
}


def scene(name):
    return _SCENES[name]


def load(name, **over):
    """The scene's data (keywords of the table, then `over`) and whether its tree is built on the GPU."""
    from pooraytracer_amd import scenes
    factory, kw, device_bvh, _ = scene(name)
    return getattr(scenes, factory)(**{**kw, **over}), device_bvh


# ---- figures

def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def rel_mse(x, ref):
    import numpy as np
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def launcher(sc, method, *args, **kw):
    """A call for `interleaved`: launches method(*args, **kw, **more), synchronises, returns the scene's counters."""
    import torch

    def go(**more):
        method(*args, **kw, **more)
        torch.cuda.synchronize()
        return sc.counters()
    return go


def interleaved(calls, launches, warmup):
    """`calls` = [(name, fn)], fn() launching, synchronising and returning counters: `warmup` rounds, then `launches` rounds
    in list order, so that a drift of the machine hits every candidate alike.  Returns {name: [kernel_ms]} and the last
    counters per name."""
    for _ in range(warmup):
        for _, fn in calls:
            fn()
    ms, last = {name: [] for name, _ in calls}, {}
    for _ in range(launches):
        for name, fn in calls:
            last[name] = fn()
            ms[name].append(last[name]["kernel_ms"])
    return ms, last


def event():
    import torch
    return torch.cuda.Event(enable_timing=True)


def timed_calls(fn, n, warm=2, after=None):
    """Wall and hipEvent milliseconds of fn(i), i = warm .. warm + n - 1, after `warm` uncounted calls (i from 0); `after()`
    runs behind every counted call, outside its timing."""
    import torch
    wall, evt = [], []
    for i in range(warm + n):
        e0, e1 = event(), event()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warm:
            wall.append(1e3 * (t1 - t0))
            evt.append(e0.elapsed_time(e1))
            if after:
                after()
    return wall, evt


def summary(wall, evt, calls=True):
    row = {"wall_ms": round(statistics.median(wall), 4), "event_ms": round(statistics.median(evt), 4),
           "wall_min_ms": round(min(wall), 4), "wall_max_ms": round(max(wall), 4)}
    if calls:
        row["calls"] = len(wall)
    return row


def emitter_mask(data):
    """True for the triangles of meshes whose material emits."""
    import numpy as np
    from pooraytracer_amd import _abi
    mask = np.zeros(data.n_tris, dtype=bool)
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DIFFUSE_LIGHT:
            mask[first[m]:first[m + 1]] = True
    return mask


def wobble(vertices, mask, amount=0.01):
    """A copy of `vertices` (triangles x 3 x 3) with the triangles of `mask` displaced sinusoidally by `amount` of their extent."""
    import numpy as np
    v = vertices.copy()
    w = vertices[mask]
    p = w.reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())
    v[mask] = w + amount * ext * np.sin(7.0 / ext * w[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3]))
    return v


def switch_blocks(sc, start, d_sets, runs, states, set_state):
    """Yields (call, {state: summary}) for refit_device and rebuild_device: at least `runs` calls per state, the states
    alternating block by block.  d_sets = (moved, start) positions on the device; a block has even length and so ends on
    the start positions, and a host refit to `start` makes the host copy current before set_state(state) (a switch refuses
    to turn on while it is stale)."""
    block = max(2, runs // 4) * 2
    for call, fn in (("refit_device", sc.refit_device), ("rebuild_device", sc.rebuild_device)):
        acc = {s: ([], []) for s in states}
        done = 0
        while done < runs:
            for state in states:
                sc.refit(start)
                set_state(state)
                wall, evt = timed_calls(lambda i: fn(d_sets[i % 2].data_ptr()), block)
                acc[state][0].extend(wall)
                acc[state][1].extend(evt)
            done += block
        yield call, {s: summary(*a) for s, a in acc.items()}


# ---- the child's half of the protocol, and the parent's

def emit(note=None, **record):
    """One JSON line on stdout for the parent; `note`, if any, on stderr for whoever watches."""
    print(json.dumps(record), flush=True)
    if note is not None:
        print(note, file=sys.stderr, flush=True)


def emit_timed(who, group, call, fn, n, warm=2, calls=True, after=None, more=None):
    """timed_calls and summary as the record {group: call, "result": row}; more() adds what the last call left behind."""
    row = summary(*timed_calls(fn, n, warm, after), calls=calls)
    row.update(more() if more else {})
    emit(f"[{who}] {call}: {row}", **{group: call}, result=row)
    return row


def collect(stdout, groups):
    """A child's JSON lines as one entry.  groups = {key: "name"} files a record {key: k, "result": r} as entry[name][k],
    {key: ("name", "second")} as entry[name][k][record[second]]; any other JSON object updates the entry itself (the header);
    lines that are no JSON object are ignored."""
    res = {(g if isinstance(g, str) else g[0]): {} for g in groups.values()}
    for line in stdout.splitlines():
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        if not isinstance(rec, dict):
            continue
        for key, g in groups.items():
            if key in rec:
                if isinstance(g, str):
                    res[g][rec[key]] = rec["result"]
                else:
                    res[g[0]].setdefault(rec[key], {})[rec[g[1]]] = rec["result"]
                break
        else:
            res.update(rec)
    return res


def spawn(argv, limit_s, tree=None, wrap=()):
    """Runs `[wrap ...] python argv` under `timeout -k 10 limit_s` with the tree (default: this one) as working directory
    and as the checkout it imports; returns (returncode, stdout).  stderr passes through."""
    tree = os.path.abspath(tree) if tree else TREE
    env = dict(os.environ, PRT_TIMING_TREE=tree) if tree != TREE else None
    r = subprocess.run(["timeout", "-k", "10", str(limit_s), *wrap, sys.executable, *argv], stdout=subprocess.PIPE, text=True,
                       cwd=tree, env=env)
    return r.returncode, r.stdout


def run_children(script, scenes, child_argv, limit_s, groups, tree=None, then=None):
    """One child `script --child <scene> child_argv` per scene, each under its own limit (limit_s, or the scene table's where
    it is None or a dict without the scene).  Returns {"scenes": {scene: entry}} with every child's records, those of a child
    that failed included; the first nonzero exit adds "failed" = {scene, returncode} and ends the run.  `then(scene, entry)`
    runs after a child that succeeded and may return such a `failed` of its own."""
    out = {"scenes": {}}
    for name in scenes:
        limit = limit_s.get(name) if isinstance(limit_s, dict) else limit_s
        rc, stdout = spawn([os.path.abspath(script), "--child", name, *child_argv], limit or scene(name)[3], tree)
        out["scenes"][name] = collect(stdout, groups)
        failed = {"scene": name, "returncode": rc} if rc != 0 else then and then(name, out["scenes"][name])
        if failed:
            out["failed"] = failed
            break  # nothing more is started after a failure
    return out


# ---- command lines and results

def common_args(ap, launches=True, runs=False, out="", worker=False):
    """--launches (refused below 10: a median needs them) and --warmup, --runs (default `runs`), --out, --child."""
    def at_least_10(text):
        if int(text) < 10:
            ap.error("--launches: the median of at least 10 launches")
        return int(text)

    if launches:
        ap.add_argument("--launches", type=at_least_10, default=11)
        ap.add_argument("--warmup", type=int, default=2)
    if runs:
        ap.add_argument("--runs", type=int, default=runs)
    ap.add_argument("--out", default=out)
    ap.add_argument("--child", *(["--worker"] if worker else []), default="", help="internal: the scene this process measures")


def scene_names(ap, text, allowed):
    names = text.split(",")
    for name in names:
        if name not in allowed:
            ap.error(f"unknown scene {name}")
    return names


def flags(args, *names):
    """The named arguments as a command line for the children: ("log2_rays",) -> ["--log2-rays", "24"]."""
    return [x for n in names for x in ("--" + n.replace("_", "-"), str(getattr(args, n)))]


def write_result(out, path):
    """Prints the result as one line and, if `path` is set, writes it there (the directory is made); the exit status."""
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    return 1 if "failed" in out else 0
