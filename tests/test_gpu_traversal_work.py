"""GPU tests (-m gpu) of the traversal WORK counters against the fp64 model of the tree walk (tests/traversal_model.py).

Every other traversal test asserts a result (hits, any-hit bytes), and the box tests are conservative: the sorting network
of inner_step, the push order, the tminf clamp, tbestf after an accept, the size of the pad, the any-hit early stop and the
place where tris_full is counted can all be wrong without any of them failing.  What they decide is how many nodes a ray
visits, and in K1 that is a function of (tree, ray) alone.  So, per case: upload with PRT_TEST_DUMP_BVH, read the tree
back, walk the batch through the model, keep the rays every decision of which is robust against the kernel's rounding,
send ONLY those with count_work and require

  node_fetches and tri_tests   == the model's sums, exactly
  tri_full                     inside the summed bracket, and == the model's on the sub-batch whose bracket is a point
  rays_closest / rays_shadow   == the batch size (the other one 0)
  hits / any-hit bytes         the model's (same primitive, t within the certifier's same-primitive tolerance)
  the sorted call's counters   == the plain call's (which also shows that counters are per call: prt_get_counters reads the
                               slot of the latest call, reset when the call takes it)

for trace_closest_device, trace_surface_device (the same walk) and trace_occluded_device, in fp64 and in fp32 (where the
tree needs at most PRT_STACK_SHALLOW stack entries the fp32 kernels walk the dumped tree with the same grid and slab_scale;
asserted).  On a failure the first offending ray is found by bisecting the batch (about 12 launches) and its visit trace in
the model is printed.

Measured nodes / ray and triangle tests / ray (kernel == model) are printed per case: DESIGN.md section 3 quotes them.
"""
import numpy as np
import pytest

from pooraytracer_amd import _abi, api
from tests import bvh_model as M
from tests import hit_certifier as H
from tests import traversal_model as T
from tests.test_gpu_occlusion import _closest, _occluded
from tests.test_gpu_surface import _surface

pytestmark = pytest.mark.gpu

STACK_SHALLOW = 32
COUNTERS = ("node_fetches", "tri_tests", "tri_full", "rays_closest", "rays_shadow")
# (scene, tree, family): host- and device-built trees on the quad scenes and the soup, inside and around; the scene at 1e6;
# one refitted tree (loosened, overlapping boxes); tmin = 0; finite intervals past several occluders
CASES = [(s, b, f) for s in ("cornell", "mixed", "soup") for b in ("host", "device") for f in ("inside", "around")] + \
    [("cornell@1e6", "host", "inside"), ("soup", "refit", "inside"), ("cornell", "host", "tmin0"), ("soup", "device", "tmin0"),
     ("mixed", "host", "segments"), ("soup", "device", "segments")]
PARAMS = [c + (p,) for c in CASES for p in ("fp64", "fp32") if not (p == "fp32" and "@" in c[0])]  # (fp32 rays do not resolve a scene at 1e6)
PRECISIONS = {"fp64": (_abi.PRECISION_F64, H.U64), "fp32": (_abi.PRECISION_F32, H.U32)}


def _jittered(vertices):
    """Every triangle moved as a whole by up to two of its extents: a refitted tree keeps its topology, its boxes overlap."""
    rng = np.random.default_rng(17)
    return vertices + rng.uniform(-0.02, 0.02, (vertices.shape[0], 1, 3))


def _resident(name, tree_kind, tmp_path, monkeypatch):
    """(scene on the GPU, its vertices as traced, the tree the kernels walk)."""
    data = T.SCENES[name]()
    path = str(tmp_path / "tree.bin")
    monkeypatch.setenv("PRT_VALIDATE_BVH", "1")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    sc = api.Scene(data, device_bvh=tree_kind == "device").upload(0)
    vertices = data.vertices
    if tree_kind == "refit":
        vertices = _jittered(data.vertices)
        sc.refit(vertices)
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    tree = M.read_dump(path)
    assert tree.built_on_device == (1 if tree_kind == "device" else 0)
    M.check_tree(tree, vertices, sc.bvh_info())
    return sc, vertices, tree


def _launch(sc, kind, rays, precision, sort=False):
    """One count_work call; returns (prim or occlusion byte, t or None, the call's counters)."""
    if kind == "occluded":
        out = _occluded(sc, rays, precision=precision, sort=sort, count_work=True)
        return out.astype(np.int64), None, sc.counters()
    fn = _closest if kind == "closest" else _surface
    h = fn(sc, rays, precision=precision, sort=sort, count_work=True)
    return h["prim"].astype(np.int64), h["t"].copy(), sc.counters()


def _mismatch(c, w, idx):
    """What of the call's counters disagrees with the model's sums over the rays `idx` ('' when nothing does)."""
    want = w.totals(idx)
    bad = [f"{k} {c[k]} != {want[k]}" for k in ("node_fetches", "tri_tests") if c[k] != want[k]]
    if not want["tri_full_lo"] <= c["tri_full"] <= want["tri_full_hi"]:
        bad.append(f"tri_full {c['tri_full']} outside [{want['tri_full_lo']}, {want['tri_full_hi']}]")
    return ", ".join(bad)


def _first_offender(sc, kind, rays, precision, w, idx):
    """Bisects the batch rays[idx] with prefix launches down to the first ray whose counts leave the model's."""
    lo, hi = 0, idx.size  # the prefix of length lo agrees, of length hi does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        _, _, c = _launch(sc, kind, rays[idx[:mid]], precision)
        if _mismatch(c, w, idx[:mid]):
            hi = mid
        else:
            lo = mid
    return int(idx[hi - 1])


def _explain(sc, kind, rays, precision, u, w, idx, tree, vertices, E, what):
    i = _first_offender(sc, kind, rays, precision, w, idx)
    _, _, c = _launch(sc, kind, rays[i:i + 1], precision)
    trace = []
    T.walk(tree, vertices, rays[i:i + 1], kind == "occluded", u, E=E, trace=trace)
    return (f"{what}\nfirst offending ray: index {i} {rays[i]!r}\nkernel alone: " + ", ".join(f"{k} {c[k]}" for k in COUNTERS) +
            f"\nmodel: nodes {w.nodes[i]} tris {w.tris[i]} tri_full [{w.full_lo[i]}, {w.full_hi[i]}]\n" + T.format_trace(trace))


@pytest.mark.parametrize("name,tree_kind,family,prec", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_work_counters_equal_the_model(dev_lib, tmp_path, monkeypatch, name, tree_kind, family, prec):
    precision, u = PRECISIONS[prec]
    sc, vertices, tree = _resident(name, tree_kind, tmp_path, monkeypatch)
    E = sc.refit_info()["slab_scale"]
    assert E == T.slab_scale(tree)
    if prec == "fp32":
        assert sc.bvh_info()["stack_need"] <= STACK_SHALLOW, "the fp32 kernels would walk the shallow collapse, not the dumped tree"
    rays = T.batch(name, family)
    n = rays.shape[0]
    rec = T.records(vertices, u)
    mag = max(1.0, float(np.abs(vertices).max()))
    # far from the origin t = (D - n.o) / (n.d) cancels |o| digits (test_gpu_device_bvh's tolerance there)
    t_tol = H.SAME_TOL[u] if mag < 1e4 else 64 * M.EPS * mag * 1e3 + 1e-12
    for any_hit, kinds in ((False, ("closest", "surface")), (True, ("occluded",))):
        w = T.walk(tree, vertices, rays, any_hit, u, E=E, rec=rec)
        idx = np.flatnonzero(w.robust)
        assert n - idx.size <= T.EXCLUDED_MAX * n, w.excluded()
        point = np.flatnonzero(w.robust & w.point)
        print(f"\n[work] {name} {tree_kind} {family} {prec} {'any-hit' if any_hit else 'closest'}: {n} rays, excluded "
              f"{n - idx.size} {w.excluded()}, point brackets {point.size}, nodes/ray {w.nodes[idx].mean():.3f} "
              f"tris/ray {w.tris[idx].mean():.3f} tri_full/ray [{w.full_lo[idx].mean():.3f}, {w.full_hi[idx].mean():.3f}]")
        for kind in kinds:
            prim, t, c = _launch(sc, kind, rays[idx], precision)
            print(f"[work]   {kind}: " + ", ".join(f"{k} {c[k]}" for k in COUNTERS))
            bad = _mismatch(c, w, idx)
            if bad:
                pytest.fail(_explain(sc, kind, rays, precision, u, w, idx, tree, vertices, E, f"{kind}: {bad}"))
            assert c["rays_shadow" if any_hit else "rays_closest"] == idx.size and c["rays_closest" if any_hit else "rays_shadow"] == 0
            if any_hit:
                assert np.array_equal(prim, (w.prim[idx] >= 0).astype(np.int64))
            else:
                assert np.array_equal(prim, w.prim[idx])
                hit = prim >= 0
                assert (np.abs(t[hit] - w.t[idx][hit]) <= t_tol * np.maximum(1.0, w.t[idx][hit])).all()
                assert np.isinf(t[~hit]).all()
            # K4's order changes which lane walks a ray, not the walk
            _, _, cs = _launch(sc, kind, rays[idx], precision, sort=True)
            assert {k: cs[k] for k in COUNTERS} == {k: c[k] for k in COUNTERS}
            # where no triangle sits at an end of its interval tri_full is exact, too
            _, _, cp = _launch(sc, kind, rays[point], precision)
            bad = _mismatch(cp, w, point)
            if bad:
                pytest.fail(_explain(sc, kind, rays, precision, u, w, point, tree, vertices, E, f"{kind}, point brackets: {bad}"))
            assert cp["tri_full"] == int(w.full_lo[point].sum()) == int(w.full_hi[point].sum())
    if "@" in name:
        # a scene far from the origin is culled as well as at the origin (the pad is relative to the grid origin)
        base = name.split("@")[0]
        monkeypatch.setenv("PRT_TEST_DUMP_BVH", str(tmp_path / "base.bin"))
        api.Scene(T.SCENES[base]()).close()
        monkeypatch.delenv("PRT_TEST_DUMP_BVH")
        w0 = T.walk(M.read_dump(str(tmp_path / "base.bin")), T.SCENES[base]().vertices, T.batch(base, family), False, u)
        w1 = T.walk(tree, vertices, rays, False, u, E=E, rec=rec)
        print(f"[work] nodes/ray {name} {w1.nodes.mean():.4f} against {base} {w0.nodes.mean():.4f}; "
              f"tris/ray {w1.tris.mean():.4f} against {w0.tris.mean():.4f}")
    sc.close()
