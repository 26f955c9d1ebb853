"""CPU tests of the fp64 model of the tree walk (tests/traversal_model.py) on host-built trees (the dev-hooks library's
PRT_TEST_DUMP_BVH dump at prt_scene_create; no GPU needed), before test_gpu_traversal_work.py holds the kernels' work
counters against it:

  a) on every robust ray the model's hit is the oracle's (same primitive, |dt| <= 1e-12 max(1, t)) and its any-hit verdict
     is the oracle's prim >= 0: the walk is pinned independently of the kernel;
  b) the model excludes at most EXCLUDED_MAX of each fixed batch, with fp64 and with fp32 margins (a condition, not a
     measurement: a batch over the cap is replaced, the cap stays);
  c) seven planted faults — the mistakes the work counters exist to catch — each change the totals of every batch they are
     claimed for, on that batch's robust rays;
  d) the order of visits on equal keys: two hand-built nodes, the order written out by hand from the network.
"""
import functools

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api
from tests import bvh_model as M
from tests import hit_certifier as H
from tests import traversal_model as T

PRECISIONS = {"fp64": H.U64, "fp32": H.U32}


@functools.lru_cache(maxsize=None)
def _tree(name):
    import os
    import tempfile
    data = T.SCENES[name]()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tree.bin")
        saved = os.environ.get("PRT_TEST_DUMP_BVH")
        os.environ["PRT_TEST_DUMP_BVH"] = path
        try:
            with api.dev_hooks():
                api.Scene(data).close()
        finally:
            if saved is None:
                del os.environ["PRT_TEST_DUMP_BVH"]
            else:
                os.environ["PRT_TEST_DUMP_BVH"] = saved
        tree = M.read_dump(path)
    M.check_tree(tree, data.vertices)
    return data, tree


@functools.lru_cache(maxsize=None)
def _walks(name, family, prec):
    """(rays, closest walk, any-hit walk) of one fixed batch, computed once and left unchanged."""
    data, tree = _tree(name)
    rays = T.batch(name, family)
    rays.setflags(write=False)
    rec = T.records(data.vertices, PRECISIONS[prec])
    return rays, T.walk(tree, data.vertices, rays, False, PRECISIONS[prec], rec=rec), T.walk(tree, data.vertices, rays, True, PRECISIONS[prec], rec=rec)


def _id(b):
    return f"{b[0]}-{b[1]}"


@pytest.mark.parametrize("name,family", T.HOST_BATCHES, ids=map(_id, T.HOST_BATCHES))
def test_robust_rays_hit_what_the_oracle_hits(prt_lib, name, family):
    data, _ = _tree(name)
    rays, closest, anyhit = _walks(name, family, "fp64")
    want = oracle.Oracle(data).trace_closest(rays)
    rb = closest.robust
    assert np.array_equal(closest.prim[rb], want["prim"][rb])
    hit = rb & (want["prim"] >= 0)
    assert hit.sum() > 100  # (the soup is sparse: 4 to 8 % of its rays hit)
    # far from the origin t = (D - n.o) / (n.d) cancels |o| digits in the oracle's doubles (test_gpu_device_bvh's tolerance)
    mag = max(1.0, float(np.abs(data.vertices).max()))
    tol = 1e-12 if mag < 1e4 else 64 * M.EPS * mag * 1e3 + 1e-12
    assert (np.abs(closest.t[hit] - want["t"][hit]) <= tol * np.maximum(1.0, want["t"][hit])).all()
    assert np.array_equal(closest.t[rb & ~hit], rays["tmax"][rb & ~hit])
    ra = anyhit.robust
    assert np.array_equal(anyhit.prim[ra] >= 0, want["prim"][ra] >= 0)
    # an any-hit walk does no more than the closest-hit one... on the rays both decide robustly, and only where it stops
    both = ra & rb & (want["prim"] < 0)
    assert np.array_equal(anyhit.nodes[both], closest.nodes[both]) and np.array_equal(anyhit.tris[both], closest.tris[both])


# (fp32 rays do not resolve a scene at 1e6: one ulp there exceeds its triangles; the fp32 kernels are not run on it)
CAP_CASES = [(n, f, p) for n, f in T.HOST_BATCHES for p in sorted(PRECISIONS) if not (p == "fp32" and "@" in n)]


@pytest.mark.parametrize("name,family,prec", CAP_CASES, ids=["-".join(c) for c in CAP_CASES])
def test_the_model_excludes_few_rays(prt_lib, capsys, name, family, prec):
    rays, closest, anyhit = _walks(name, family, prec)
    n = rays.shape[0]
    for kind, w in (("closest", closest), ("any-hit", anyhit)):
        wide = float((~w.point & w.robust).mean())
        print(f"[work-model] {name} {family} {prec} {kind}: {n} rays, excluded {int((~w.robust).sum())} {w.excluded()}, "
              f"tri_full bracket wider than a point on {100 * wide:.1f} % of the rays, "
              f"nodes/ray {w.nodes[w.robust].mean():.3f} tris/ray {w.tris[w.robust].mean():.3f}")
        assert (~w.robust).sum() <= T.EXCLUDED_MAX * n, w.excluded()
        assert (w.full_lo <= w.full_hi).all() and (w.full_hi <= w.tris).all() and (w.nodes >= 1).all()
    out = capsys.readouterr().out
    assert out.count("tri_full bracket wider than a point on") == 2  # the share of bracketed rays is reported, per walk
    print(out, end="")  # back into the captured output (pytest -rP shows it)


# ------------------------------------------------------------------------------------------------------ planted faults
# fault -> the walks it is claimed for.  tbestf only matters after an accept that does not end the walk (closest hit); the
# early stop exists only in an any-hit walk; everything else shows in both.
CLAIMS = {"no_tbestf": ("closest",), "no_any_stop": ("any-hit",), "drop_last_ce": ("closest", "any-hit"),
          "push_reversed": ("closest", "any-hit"), "pad_x16": ("closest", "any-hit"), "no_tminf": ("closest", "any-hit"),
          "full_before_interval": ("closest", "any-hit")}
COUNTERS = {"full_before_interval": ("tri_full_lo", "tri_full_hi")}  # every other fault: node_fetches and tri_tests


@pytest.mark.parametrize("fault", T.FAULTS)
def test_planted_faults_change_the_totals_of_every_batch(prt_lib, fault):
    assert set(CLAIMS) == set(T.FAULTS)
    for name, family in T.HOST_BATCHES:
        data, tree = _tree(name)
        rays, closest, anyhit = _walks(name, family, "fp64")
        rec = T.records(data.vertices, H.U64)
        for kind, w in (("closest", closest), ("any-hit", anyhit)):
            if kind not in CLAIMS[fault]:
                continue
            bad = T.walk(tree, data.vertices, rays, kind == "any-hit", H.U64, faults=(fault,), rec=rec)
            a, b = w.totals(), bad.totals(w.robust)
            keys = COUNTERS.get(fault, ("node_fetches", "tri_tests"))
            rel = {k: (b[k] - a[k]) / max(a[k], 1) for k in keys}
            print(f"\n[work-model] {fault} on {name} {family} {kind}: " + ", ".join(f"{k} {a[k]} -> {b[k]} ({100 * rel[k]:+.3f} %)" for k in keys))
            if fault == "full_before_interval":
                # counted before the interval check, tri_full leaves the bracket: above its upper end
                assert b["tri_full_lo"] > a["tri_full_hi"]
            else:
                # the GPU test asserts both counters exactly: a fault shows when either total moves
                assert (b["node_fetches"], b["tri_tests"]) != (a["node_fetches"], a["tri_tests"])
                if fault in ("no_tbestf", "no_any_stop", "pad_x16", "no_tminf"):  # these can only add work
                    assert b["node_fetches"] >= a["node_fetches"] and b["tri_tests"] >= a["tri_tests"]
                    assert b["node_fetches"] + b["tri_tests"] > a["node_fetches"] + a["tri_tests"]


# ------------------------------------------------------------------------------------------------------------ tie rule
def _node_tree(children):
    """One 4-wide node over a unit grid (origin 0, step 2^-12: boxes are exact): children = [((lo, hi) per axis in grid
    units, triangle)], each a one-triangle leaf."""
    nodes = np.zeros(1, dtype=M.NODE)
    for f in ("bx", "by", "bz"):
        nodes[f][0, :] = M.INVERTED
    nodes["ref"][0, :] = M.UNUSED
    for s, (box, tri) in enumerate(children):
        for f, (lo, hi) in zip(("bx", "by", "bz"), box):
            nodes[f][0, s] = lo | (hi << 16)
        nodes["ref"][0, s] = ~np.int32(tri << 3)
    n = len(children)
    step = 2.0 ** -12
    return M.Tree(n, 0, 1, n - 1, (0.0, 0.0, 0.0), (step, step, step), 16.0, nodes, np.arange(n))


def _leaf_order(tree, vertices, ray):
    trace = []
    w = T.walk(tree, vertices, ray, trace=trace)
    assert w.robust.all(), w.excluded()
    leaves = [(~ev[1] & 0xFFFFFFFF) >> 3 for ev in trace if ev[0] == "leaf"]
    print("\n" + T.format_trace(trace))
    return leaves, w


def _far_triangles(n):
    """n triangles nowhere near the rays (the leaves are visited, their triangles missed)."""
    v = np.zeros((n, 3, 3))
    v[:, :, 1] = 100.0 + np.arange(n)[:, None]
    v[:, 1, 0] = v[:, 2, 2] = 1.0
    return v


def _ray(o, d, tmin=1e-4):
    r = np.zeros(1, dtype=_abi.RAY_DTYPE)
    r["o"], r["d"], r["tmin"], r["tmax"] = o, d, tmin, np.inf
    return r


def test_children_sharing_an_entry_plane_are_visited_in_the_networks_order():
    """Slots 0..3: A and C and D enter through the plane x = 1024 steps (bit-identical keys), B through x = 512 steps.
    Keys (k0..k3) = (e, b, e, e), b < e.  The network: (0,1) swaps -> B A C D; (2,3) e < e is false; (0,2) e < b is false;
    (1,3) and (1,2) e < e are false.  Visit order B A C D: equal keys keep their slots' order."""
    yz = ((1024, 3072), (1024, 3072))
    tree = _node_tree([(((1024, 2048),) + yz, 0), (((512, 900),) + yz, 1), (((1024, 1500),) + yz, 2), (((1024, 3000),) + yz, 3)])
    step = 2.0 ** -12
    leaves, w = _leaf_order(tree, _far_triangles(4), _ray((-0.25, 2000.5 * step, 2100.25 * step), (1.0, 0.0, 0.0)))
    assert leaves == [1, 0, 2, 3]
    assert w.nodes[0] == 1 and w.tris[0] == 4
    # the same boxes with B in slot 3: slots (A, C, D, B), keys (e, e, e, b).  (0,1) no; (2,3) b < e swaps -> (A, C, B, D);
    # (0,2) b < e swaps -> (B, C, A, D); (1,3) and (1,2) e < e are false.  Visit order B C A D = triangles 3 1 0 2.
    tree = _node_tree([(((1024, 2048),) + yz, 0), (((1024, 1500),) + yz, 1), (((1024, 3000),) + yz, 2), (((512, 900),) + yz, 3)])
    leaves, _ = _leaf_order(tree, _far_triangles(4), _ray((-0.25, 2000.5 * step, 2100.25 * step), (1.0, 0.0, 0.0)))
    assert leaves == [3, 1, 0, 2]


def test_children_that_all_contain_the_origin_are_visited_in_slot_order():
    """Every entry distance is clamped to tminf: four equal keys, no compare-exchange swaps, visit order 0 1 2 3 — with
    tmin = 1e-4 and with tmin = 0 (the clamp is +0).  Without the clamp (the planted fault) the negative entry distances
    order as unsigned integers: the farthest plane behind the origin first."""
    box = ((1000, 3000), (1000, 3000), (1000, 3000))
    grow = lambda k: tuple((lo - 100 * k, hi + 100 * k) for lo, hi in box)  # noqa: E731
    tree = _node_tree([(grow(2), 0), (grow(0), 1), (grow(3), 2), (grow(1), 3)])
    step = 2.0 ** -12
    o = (2000.5 * step, 2100.25 * step, 1900.75 * step)
    for tmin in (1e-4, 0.0):
        leaves, w = _leaf_order(tree, _far_triangles(4), _ray(o, (0.6, 0.0, 0.8), tmin))
        assert leaves == [0, 1, 2, 3] and w.nodes[0] == 1
    trace = []
    T.walk(tree, _far_triangles(4), _ray(o, (0.6, 0.0, 0.8)), faults=("no_tminf",), trace=trace)
    # entry distances -a < 0: as unsigned integers a larger |a| is a LARGER key; the nearest plane behind the origin is
    # the smallest box's (slot 1), then slots 3, 0, 2
    assert [(~ev[1] & 0xFFFFFFFF) >> 3 for ev in trace if ev[0] == "leaf"] == [1, 3, 0, 2]
