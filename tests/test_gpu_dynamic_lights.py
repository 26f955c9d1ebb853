"""GPU tests (-m gpu) of moving emitters under a refit or a rebuild (prt_scene_set_dynamic_lights, include/prt.h; the table
kernels in light_tables.hip): after every motion the light state of the resident scene is the one a fresh scene of the new
vertices has — CDF order, picks and table words bit for bit — and the oracle's.

Cases (what matters is the triangle count of each emissive mesh, not the frame):
  A  one emissive mesh of 16 triangles over a floor: the smallest table, under the span-1 wrap-around node of a one-mesh list
  B  15 triangles: no table, the tree only
  C  two emissive meshes, 40 and 2 triangles
  D  three meshes, 17 / 33 / 300: odd spans
  E  scenes.veach_mis(64, 36): 6,400 emitter triangles in five meshes
Motions, each from the start positions and applied to emitters and non-emitters alike: a translation, a per-mesh anisotropic
scale (the dominant axis, hence the sort keys, change), a 90 degree rotation about y, a per-vertex jitter of 1 % of the extent
(the areas change), and the way back.  Through refit, refit_device, rebuild and rebuild_device, both builders.

The oracle's results per (case, motion) are computed once and shared by the entry points.

Three notes on the cases.  (1) A lights list of exactly two meshes is one clean subtree, so C carries ONE table at the
root; a one-mesh list (A, and the layout test) has a span-1 node above its table, and so has every list of three or more
meshes somewhere (note 3): D has two tables, veach-mis three.  (2) Because C's root is clean, a collapsed
40-triangle mesh beside a 2-triangle one leaves the root's area positive and the plan unchanged: the layout exception
(a subtree whose bucket width is not finite) is reached here by collapsing the only emissive mesh of a one-mesh scene.
(3) A lights list of three or more meshes is sorted by position and split at its middle, so WHICH mesh ends up alone
in a span-1 node - the node the wrap-around makes unclean, below which the tables start - follows the motion: D and E change
their table layout under some motions (relaid = 1), and their LDS sizing is then compared with the fresh scene's.
The environment hook of the verification-failure test is set the way this suite sets its other hooks: in the process, on
the dev-hooks library, which reads it at the call."""
import copy
import functools

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, scenes
from tests.test_gpu_f32 import trace
from tests.test_gpu_parity import compare_images

pytestmark = pytest.mark.gpu

RENDER = dict(spp=4, max_depth=8, seed=2)


def _patch(n, center, size, seed):
    """n triangles of a slightly crumpled, downward-facing grid patch around `center`."""
    cells = 1
    while 2 * cells * cells < n:
        cells += 1
    rng = np.random.default_rng(seed)
    bump = rng.uniform(-0.05, 0.05, size=(cells + 1, cells + 1)) * size
    c = np.asarray(center, dtype=np.float64)
    v, uv = scenes.grid_quad(c + np.array([-size / 2, 0.0, -size / 2]), (size, 0.0, 0.0), (0.0, 0.0, size), cells, cells,
                             displace=lambda s, t: bump)
    keep = rng.permutation(v.shape[0])[:n]
    return v[keep], uv[keep]


def _lit_floor(name, lights, width=24, height=24):
    b = scenes._Builder(name)
    white = b.material(scenes.Material("white", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    b.mesh("floor", white, *scenes.quad((-2, -1, 2), (2, -1, 2), (2, -1, -2), (-2, -1, -2)))
    b.mesh("block", white, *scenes.box((-0.4, -0.8, -0.4), (0.3, -0.3, 0.3)))
    for k, (n, center, size) in enumerate(lights):
        m = b.material(scenes.Material(f"light{k + 1}", _abi.MAT_DIFFUSE_LIGHT, emission=(6.0 + 3 * k, 5.0, 4.0 - k)))
        b.mesh(f"light{k + 1}", m, *_patch(n, center, size, seed=10 + k))
    return b.build(scenes.Camera(width, height, 40.0, eye=(0.0, 1.5, 5.0), look_at=(0.0, -0.5, 0.0)))


CASES = {
    "A": lambda: _lit_floor("A", [(16, (0.0, 1.0, 0.0), 0.8)]),
    "B": lambda: _lit_floor("B", [(15, (0.0, 1.0, 0.0), 0.8)]),
    "C": lambda: _lit_floor("C", [(40, (-0.6, 1.0, 0.1), 0.7), (2, (0.9, 0.8, -0.3), 0.4)]),
    "D": lambda: _lit_floor("D", [(17, (-1.0, 1.0, 0.0), 0.5), (33, (0.1, 1.2, 0.5), 0.6), (300, (1.0, 0.9, -0.4), 0.9)]),
    "E": lambda: scenes.veach_mis(64, 36),
}
N_ORIGINS = {"A": 20_000, "B": 20_000, "C": 20_000, "D": 20_000, "E": 200_000}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def emissive(data):
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    mask = np.zeros(data.n_tris, dtype=bool)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DIFFUSE_LIGHT:
            mask[first[m]:first[m + 1]] = True
    return mask


def translate(data):
    return data.vertices + np.array([0.3, -0.2, 0.5])


def scale(data):
    """The per-mesh anisotropic scale of test_update_vertices_rebuilds_the_light_tables, on every mesh."""
    v = data.vertices.copy()
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for k in range(len(data.mesh_material)):
        sl = slice(first[k], first[k + 1])
        c = v[sl].reshape(-1, 3).mean(0)
        v[sl] = (v[sl] - c) * np.array([1.0 + 0.35 * (k % 4), 0.8, 1.1 + 0.1 * (k % 4)]) + c + np.array([0.02 * k, 0.05, -0.03])
    return v


def rotate(data):
    v = data.vertices
    return np.ascontiguousarray(np.stack([v[..., 2], v[..., 1], -v[..., 0]], axis=-1))


def jitter(data):
    lo, hi = data.bounds()
    return data.vertices + np.random.default_rng(3).uniform(-1.0, 1.0, size=data.vertices.shape) * 0.01 * float((hi - lo).max())


def back(data):
    return data.vertices.copy()


MOTIONS = [("translate", translate), ("scale", scale), ("rotate", rotate), ("jitter", jitter), ("back", back)]


def with_vertices(data, v):
    out = copy.copy(data)
    out.vertices = v
    return out


@functools.lru_cache(maxsize=None)
def moved_vertices(name, tag):
    v = np.ascontiguousarray(dict(MOTIONS)[tag](case(name)))
    v.setflags(write=False)
    return v


def origins(name):
    return np.random.default_rng(5).uniform(-3, 3, size=(N_ORIGINS[name], 3))


@functools.lru_cache(maxsize=None)
def oracle_reference(name, tag):
    """The oracle's light order, picks and frame of the moved scene: computed once per (case, motion)."""
    orc = oracle.Oracle(with_vertices(case(name), moved_vertices(name, tag)))
    frame, _ = orc.render(**RENDER)
    return orc.light_order(), orc.sample_lights(origins(name), seed=9), frame


ENTRIES = ["refit", "refit_device", "rebuild", "rebuild_device"]
BUILDERS = [pytest.param(False, id="host"), pytest.param(True, id="device")]


def move(sc, entry, v, normals):
    """The scene's positions become `v` through one of the four entry points (the device forms from torch tensors)."""
    v = np.ascontiguousarray(v)
    if entry in ("refit", "rebuild"):
        getattr(sc, entry)(v, normals=normals)
        return
    import torch
    d_v = torch.from_numpy(v.copy()).cuda()
    d_n = None if normals is None else torch.from_numpy(np.ascontiguousarray(normals)).cuda()
    torch.cuda.synchronize()
    getattr(sc, entry)(d_v.data_ptr(), None if d_n is None else d_n.data_ptr())
    torch.cuda.synchronize()


def assert_same_picks(g, c, label, exact_positions):
    assert np.array_equal(g["prim"], c["prim"]) and np.array_equal(g["front"], c["front"]), label
    assert np.array_equal(g["pdf"].view(np.uint64), c["pdf"].view(np.uint64)), label
    if exact_positions:
        assert np.array_equal(g["position"].view(np.uint64), c["position"].view(np.uint64)), label
        assert np.array_equal(g["normal"].view(np.uint64), c["normal"].view(np.uint64)), label
    else:
        assert np.abs(g["position"] - c["position"]).max() <= 1e-13 * max(1.0, np.abs(c["position"]).max()), label


LDS_FIELDS = ("lds_light_nodes", "lds_light_tris", "render_variant")


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(CASES))
def test_light_state_follows_every_motion(gpu, name, entry, device_bvh):
    """After each motion: light_order, sample_lights and the frame are the oracle's for the moved scene; order, picks (every
    bit) and table words are a fresh scene's; the LDS sizing is untouched while the layout is; updates counts the calls
    that moved an emitter, and a call that moves only the rest leaves the light words alone."""
    data = case(name)
    org = origins(name)
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    assert not sc.dynamic_lights
    sc.dynamic_lights = True
    assert sc.dynamic_lights
    words0, info0 = sc.light_table_words(), sc.bvh_info()
    assert (words0.size > 0) == (name != "B")
    assert sc.light_update_info()["updates"] == 0
    for step, (tag, _) in enumerate(MOTIONS):
        v = moved_vertices(name, tag)
        label = f"{name} {entry} {tag}"
        move(sc, entry, v, data.normals)
        lu = sc.light_update_info()
        print(f"[lights] {label}: gather {lu['gather_ms']:.3f} ms, host tree {lu['host_tree_ms']:.3f} ms, tables {lu['tables_ms']:.3f} ms, "
              f"{lu['n_tables']} tables / {lu['table_words']} words")
        assert lu["updates"] == step + 1 and lu["tables_dropped"] == 0, (label, lu)
        if name in "ABC":  # one or two light meshes: no motion changes the layout (three or more: see the module's note 3)
            assert lu["relaid"] == 0, (label, lu)
        order_ref, picks_ref, frame_ref = oracle_reference(name, tag)
        fresh = api.Scene(with_vertices(data, v)).upload(gpu)
        order = sc.light_order()
        assert np.array_equal(order, order_ref) and np.array_equal(order, fresh.light_order()), label
        picks = sc.sample_lights(org, seed=9)
        assert_same_picks(picks, picks_ref, label + " vs oracle", exact_positions=False)
        assert_same_picks(picks, fresh.sample_lights(org, seed=9), label + " vs fresh", exact_positions=True)
        words = sc.light_table_words()
        assert np.array_equal(words, fresh.light_table_words()), label
        if tag == "back":
            assert np.array_equal(words, words0), label
        info, want = sc.bvh_info(), info0 if lu["relaid"] == 0 else fresh.bvh_info()
        for f in LDS_FIELDS:
            assert info[f] == want[f], (label, f)
        compare_images(sc.render(**RENDER), frame_ref)
        fresh.close()
    # a call that moves only non-emitters: no light update, the light words stay bit-equal
    v = data.vertices.copy()
    v[~emissive(data)] += np.array([0.0, -0.01, 0.0])
    move(sc, entry, v, data.normals)
    assert sc.light_update_info()["updates"] == len(MOTIONS)
    assert np.array_equal(sc.light_table_words(), words0)
    for f in LDS_FIELDS:
        assert sc.bvh_info()[f] == info0[f], f
    assert np.array_equal(sc.light_order(), oracle_reference(name, "back")[0])
    sc.close()


F32 = dict(spp=8, max_depth=6, seed=4, precision=_abi.PRECISION_F32)


@functools.lru_cache(maxsize=None)
def fresh_f32_frame(name, tag):
    """The PRT_PRECISION_F32 frame of a fresh scene of the moved vertices: rendered once per (case, motion)."""
    fresh = api.Scene(with_vertices(case(name), moved_vertices(name, tag))).upload(0)
    frame = fresh.render(**F32)
    fresh.close()
    return frame


def f32_tables(sc):
    """Makes the scene's fp32 tables without a frame: a few rays through the fp32 batch kernel."""
    lo, hi = sc.data.bounds()
    trace(sc, scenes.random_rays(64, lo, hi, seed=1), _abi.PRECISION_F32)
    assert sc.bvh_info()["render_variant"] >> 8


def assert_f32_frame(got, want, label):
    """Second tolerance tier, the figures of test_gpu_f32: the frame is finite, its mean within 1e-3 of the fresh scene's, and
    at most 1 % of the pixels differ by more than 1e-3 max(1, |value|) (the two scenes traverse trees of different topology,
    and fp32 hits are not tree-independent to the last bit)."""
    assert np.isfinite(got).all(), label
    far = (np.abs(got - want) > 1e-3 * np.maximum(1.0, np.abs(want))).any(-1)
    print(f"[lights] fp32 {label}: {int(far.sum())} of {far.size} pixels far, mean ratio {got.mean() / want.mean():.6f}")
    assert abs(got.mean() - want.mean()) <= 1e-3 * want.mean(), label
    assert far.mean() <= 0.01, (label, float(far.mean()))


@pytest.mark.parametrize("tables_first", [False, True], ids=["tables_after", "tables_before"])
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_frames_follow_every_motion(gpu, name, entry, device_bvh, tables_first):
    """PRT_PRECISION_F32 on the updated scene against PRT_PRECISION_F32 on a fresh scene of the moved vertices, after every
    motion in sequence (so every update after the first finds fp32 light copies in both the resident and the spare arrays,
    and D and E go through updates that change the layout), with the fp32 tables made before the first move (the light ones
    are re-derived by each update) or after it (they are derived from the updated state)."""
    data = case(name)
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    sc.dynamic_lights = True
    if tables_first:
        sc.render(**F32)
        assert sc.bvh_info()["render_variant"] >> 8
    for step, (tag, _) in enumerate(MOTIONS):
        move(sc, entry, moved_vertices(name, tag), data.normals)
        assert sc.light_update_info()["updates"] == step + 1
        assert_f32_frame(sc.render(**F32), fresh_f32_frame(name, tag), f"{name} {entry} {tag} tables_first={tables_first}")
    sc.close()


def chain_motions(data):
    """The chain of test_every_follower_through_a_chain_of_motions: (entry point, tag, vertices), each motion from the start
    positions and each a pure function of position within a mesh, so that bitwise-welded corners stay welded (the signed
    tables' ids are made at upload and kept)."""
    from tests.test_gpu_signed_distance import wobble
    return [("refit_device", "translate", translate(data)), ("rebuild", "scale", scale(data)), ("refit", "wobble", wobble(data.vertices)),
            ("rebuild_device", "rotate", rotate(data)), ("refit", "back", back(data))]


def follower_scene(data, device_bvh):
    """Every follower of the geometry resident at once: dynamic lights, signed (hence distance) queries, the fp32 tables."""
    sc = api.Scene(data, device_bvh=device_bvh)
    sc.dynamic_lights = True
    sc.signed_queries = True
    sc.upload(0)
    sc.render(**F32)
    assert sc.distance_queries is True and sc.bvh_info()["render_variant"] >> 8
    return sc


@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_every_follower_through_a_chain_of_motions(gpu, device_bvh):
    """Case D with dynamic lights, signed queries and the fp32 tables resident, through refit_device -> rebuild -> refit ->
    rebuild_device -> refit on ONE scene (each path inherits what the previous one left: the rebuild replaces the refit's
    parents and counters, drops the shallow tree and sizes both kernel configs again).  After each step the scene is a fresh
    scene's of the same vertices, builder and switches, each quantity by the comparison of its own per-feature test: light
    order, table words, picks, pseudonormals, signed and closest-point records bit for bit; fp64 hits within the hit
    tolerance; fp32 hits at tier 2; the fp64 frame within 1e-9 on every pixel; the fp32 frame at the second tier."""
    from tests import signed_distance_model as SM
    from tests.closest_point_model import queries
    from tests.test_gpu_refit import assert_same_hits, assert_same_hits_tier2, trace_dev
    from tests.test_gpu_signed_distance import check_contract
    data = case("D")
    org = origins("D")
    welds = SM.topology(data.vertices)["info"]
    q = queries(data.vertices, 1024, 77)
    p = np.ascontiguousarray(np.concatenate([q["near"][0], q["box"][0]]))
    assert p.shape[0] == 2048
    sc = follower_scene(data, device_bvh)
    refits = sc.refit_info()["refits"]
    for step, (entry, tag, v) in enumerate(chain_motions(data)):
        label = f"D {step} {entry} {tag}"
        v = np.ascontiguousarray(v)
        assert SM.topology(v)["info"] == welds, label  # the welds survived
        move(sc, entry, v, data.normals)
        refits += entry.startswith("refit")
        info = sc.refit_info()
        assert info["refits"] == refits, label
        assert info["host_stale"] == (1 if entry.endswith("_device") else 0), label
        assert sc.light_update_info()["updates"] == step + 1, label
        assert sc.signed_queries is True and sc.distance_queries is True and sc.dynamic_lights is True
        fresh = follower_scene(with_vertices(data, v), device_bvh)
        assert np.array_equal(sc.light_order(), fresh.light_order()), label
        assert np.array_equal(sc.light_table_words(), fresh.light_table_words()), label
        assert_same_picks(sc.sample_lights(org, seed=9), fresh.sample_lights(org, seed=9), label, exact_positions=True)
        P = fresh.pseudonormals()
        assert sc.pseudonormals().tobytes() == P.tobytes(), label
        signed, closest = sc.signed_distance(p), sc.closest_point(p)
        assert signed.tobytes() == fresh.signed_distance(p).tobytes(), label
        assert closest.tobytes() == fresh.closest_point(p).tobytes(), label
        check_contract(signed, closest, p, v, P, label)
        lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
        pad = 0.25 * np.maximum(hi - lo, 1e-3)
        rays = scenes.random_rays(2000, lo - pad, hi + pad, seed=6 + step)
        (g, go), (r, ro) = trace_dev(sc, rays), trace_dev(fresh, rays)
        assert np.array_equal(go, ro), label
        assert_same_hits(g, r, rays, v, label)
        (g, go), (r, ro) = trace_dev(sc, rays, precision=_abi.PRECISION_F32), trace_dev(fresh, rays, precision=_abi.PRECISION_F32)
        assert_same_hits_tier2(g, r, rays, v, label, "D")
        assert (go != ro).sum() <= 1e-4 * rays.shape[0], label
        compare_images(sc.render(**RENDER), fresh.render(**RENDER), max_bad=0)
        assert_f32_frame(sc.render(**F32), fresh.render(**F32), label)
        fresh.close()
    sc.close()


def test_switch_off_refuses_a_moved_emitter_as_before(gpu):
    """The default: a moved emitter vertex is PRT_E_INVALID with today's message through all four entry points, and frames,
    picks and table words stay bit-equal."""
    data = case("C")
    sc = api.Scene(data).upload(gpu)
    assert sc.dynamic_lights is False
    org = origins("C")
    frame0, picks0, words0 = sc.render(**RENDER), sc.sample_lights(org, seed=9), sc.light_table_words()
    info0 = sc.refit_info()
    for entry in ENTRIES:
        with pytest.raises(api.PrtError) as e:
            move(sc, entry, moved_vertices("C", "translate"), data.normals)
        assert e.value.code == _abi.PRT_E_INVALID and "a vertex of a light mesh moved" in str(e.value) and "prt_scene_update_vertices" in str(e.value)
        assert np.array_equal(sc.render(**RENDER), frame0) and np.array_equal(sc.sample_lights(org, seed=9), picks0), entry
        assert np.array_equal(sc.light_table_words(), words0) and sc.refit_info() == info0, entry
    assert sc.light_update_info()["updates"] == 0
    sc.close()


def test_a_refused_call_changes_no_light_word(gpu):
    """Switch on, emitters moved, and a NaN on a non-emitter vertex: PRT_E_INVALID, and no light word, pick or frame changes;
    the next good call then updates the lights."""
    data = case("D")
    sc = api.Scene(data).upload(gpu)
    sc.dynamic_lights = True
    org = origins("D")
    frame0, picks0, words0, order0 = sc.render(**RENDER), sc.sample_lights(org, seed=9), sc.light_table_words(), sc.light_order()
    info0 = sc.refit_info()
    v = moved_vertices("D", "jitter").copy()
    v[np.nonzero(~emissive(data))[0][3], 1, 2] = np.nan
    for entry in ENTRIES:
        with pytest.raises(api.PrtError) as e:
            move(sc, entry, v, data.normals)
        assert e.value.code == _abi.PRT_E_INVALID and "not finite" in str(e.value), entry
        assert np.array_equal(sc.light_table_words(), words0) and np.array_equal(sc.light_order(), order0), entry
        assert np.array_equal(sc.sample_lights(org, seed=9), picks0) and np.array_equal(sc.render(**RENDER), frame0), entry
        assert sc.refit_info() == info0 and sc.light_update_info()["updates"] == 0, entry
    move(sc, "refit", moved_vertices("D", "jitter"), data.normals)
    assert sc.light_update_info()["updates"] == 1
    assert np.array_equal(sc.light_order(), oracle_reference("D", "jitter")[0])
    sc.close()


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_failure_while_staging_puts_everything_back(dev_lib, monkeypatch, entry, k):
    """PRT_TEST_FAIL_LIGHT_STAGE=k (dev-hooks library): the k-th allocation of the spare light arrays (nodes, records, table
    words, and the two fp32 copies: the fp32 tables exist) reports out-of-memory AFTER the host has recomputed the emitter
    triangles and the light tree.  PRT_E_OOM, and nothing changed: light words, order, picks, frame, refit_info, and the
    emitters' host records - a fresh upload of the scene's host state renders the start frame bit for bit.  The next call,
    without the hook, updates the lights."""
    data = case("D")
    sc = api.Scene(data).upload(0)
    sc.dynamic_lights = True
    sc.render(**F32)
    org = origins("D")
    frame0, picks0, words0, order0 = sc.render(**RENDER), sc.sample_lights(org, seed=9), sc.light_table_words(), sc.light_order()
    info0 = sc.refit_info()
    monkeypatch.setenv("PRT_TEST_FAIL_LIGHT_STAGE", str(k))
    with pytest.raises(api.PrtError) as e:
        move(sc, entry, moved_vertices("D", "jitter"), data.normals)
    monkeypatch.delenv("PRT_TEST_FAIL_LIGHT_STAGE")
    assert e.value.code == _abi.PRT_E_OOM and "PRT_TEST_FAIL_LIGHT_STAGE" in str(e.value)
    assert np.array_equal(sc.light_table_words(), words0) and np.array_equal(sc.light_order(), order0)
    assert np.array_equal(sc.sample_lights(org, seed=9), picks0) and np.array_equal(sc.render(**RENDER), frame0)
    assert sc.refit_info() == info0 and sc.light_update_info()["updates"] == 0
    sc.upload(0)  # from the host records: the emitters' are the start's again
    sc.render(**F32)
    assert np.array_equal(sc.render(**RENDER), frame0) and np.array_equal(sc.sample_lights(org, seed=9), picks0)
    move(sc, entry, moved_vertices("D", "jitter"), data.normals)
    assert sc.light_update_info()["updates"] == 1
    assert np.array_equal(sc.light_order(), oracle_reference("D", "jitter")[0])
    assert_same_picks(sc.sample_lights(org, seed=9), oracle_reference("D", "jitter")[1], "after the failure", exact_positions=False)
    sc.close()


@pytest.mark.parametrize("entry", ["refit_device", "rebuild"])
def test_a_failed_verification_keeps_the_full_tree(dev_lib, monkeypatch, entry):
    """PRT_TEST_FAIL_LIGHT_VERIFY=1 (dev-hooks library): after the move the scene descends the full tree — no table words,
    tables_dropped and relaid set, the kernels sized again — and the picks are still the oracle's bit for bit, the frame
    within 1e-9.  Without the hook the next update brings the tables back."""
    data = case("D")
    sc = api.Scene(data).upload(0)
    sc.dynamic_lights = True
    assert sc.light_table_words().size > 0
    sc.render(**F32)  # the fp32 tables exist: every update below re-derives the light ones
    extra0 = sc.bvh_info()["render_variant"] & _abi.VARIANT_EXTRA
    monkeypatch.setenv("PRT_TEST_FAIL_LIGHT_VERIFY", "1")
    move(sc, entry, moved_vertices("D", "scale"), data.normals)
    monkeypatch.delenv("PRT_TEST_FAIL_LIGHT_VERIFY")
    lu = sc.light_update_info()
    assert lu["updates"] == 1 and lu["tables_dropped"] == 1 and lu["relaid"] == 1 and lu["n_tables"] == 0 and lu["table_words"] == 0
    assert sc.light_table_words().size == 0
    assert extra0 and not (sc.bvh_info()["render_variant"] & _abi.VARIANT_EXTRA)
    order_ref, picks_ref, frame_ref = oracle_reference("D", "scale")
    assert np.array_equal(sc.light_order(), order_ref)
    assert_same_picks(sc.sample_lights(origins("D"), seed=9), picks_ref, "full tree", exact_positions=False)
    compare_images(sc.render(**RENDER), frame_ref)
    assert_f32_frame(sc.render(**F32), fresh_f32_frame("D", "scale"), f"{entry} tables dropped")
    move(sc, entry, moved_vertices("D", "rotate"), data.normals)
    lu = sc.light_update_info()
    assert lu["updates"] == 2 and lu["tables_dropped"] == 0 and lu["relaid"] == 1 and lu["n_tables"] >= 1
    fresh = api.Scene(with_vertices(data, moved_vertices("D", "rotate"))).upload(0)
    assert np.array_equal(sc.light_table_words(), fresh.light_table_words())
    assert_same_picks(sc.sample_lights(origins("D"), seed=9), oracle_reference("D", "rotate")[1], "tables back", exact_positions=False)
    assert_f32_frame(sc.render(**F32), fresh_f32_frame("D", "rotate"), f"{entry} tables back")
    sc.close()
    fresh.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_layout_exception_agrees_with_a_fresh_scene(gpu, entry):
    """The only emissive mesh (40 triangles) collapses onto one point: its area is 0, the bucket width of its table is not
    finite, and the plan gives no table.  relaid is 1; order, words and picks are what the library's own create path makes
    of the same degenerate input.  A move back restores the original words (relaid again), the fp64 frame and - the fp32
    tables exist from the start and are re-derived by both updates - the fp32 frame.  (No frame is taken of the collapsed
    state: its total light area is 0 and every pdf a NaN, in the fresh scene as well.)"""
    data = _lit_floor("one40", [(40, (0.0, 1.0, 0.0), 0.8)])
    sc = api.Scene(data).upload(gpu)
    sc.dynamic_lights = True
    f32_0 = api.Scene(data).upload(gpu).render(**F32)
    sc.render(**F32)
    words0, info0 = sc.light_table_words(), sc.bvh_info()
    assert words0.size > 0
    org = origins("A")
    v = data.vertices.copy()
    v[emissive(data)] = np.array([0.1, 1.0, -0.2])
    move(sc, entry, v, data.normals)
    lu = sc.light_update_info()
    assert lu["updates"] == 1 and lu["relaid"] == 1 and lu["tables_dropped"] == 0 and lu["n_tables"] == 0
    fresh = api.Scene(with_vertices(data, v)).upload(gpu)
    assert fresh.light_table_words().size == 0 and sc.light_table_words().size == 0
    assert np.array_equal(sc.light_order(), fresh.light_order())
    g, c = sc.sample_lights(org, seed=9), fresh.sample_lights(org, seed=9)
    assert g.tobytes() == c.tobytes()
    f32_tables(fresh)  # (so that both precisions' sizing is compared: sc has had its fp32 tables from the start)
    for f in LDS_FIELDS:
        assert sc.bvh_info()[f] == fresh.bvh_info()[f], f
    fresh.close()
    move(sc, entry, data.vertices.copy(), data.normals)
    lu = sc.light_update_info()
    assert lu["updates"] == 2 and lu["relaid"] == 1 and lu["n_tables"] == 1
    assert np.array_equal(sc.light_table_words(), words0)
    for f in LDS_FIELDS:
        assert sc.bvh_info()[f] == info0[f], f
    compare_images(sc.render(**RENDER), oracle.Oracle(data).render(**RENDER)[0])
    assert_f32_frame(sc.render(**F32), f32_0, f"{entry} back from the collapse")
    sc.close()


def test_ordering_against_calls_in_flight(gpu):
    """render_device on stream A, refit_device with moved lights on stream B, render_device on stream A into a second
    buffer: the first frame is lit by the old lights, the second by the new ones (both against fresh scenes, 1e-9).  A light
    update there and back beforehand leaves this one nothing to allocate."""
    import torch
    data = _lit_floor("D256", [(17, (-1.0, 1.0, 0.0), 0.5), (33, (0.1, 1.2, 0.5), 0.6), (300, (1.0, 0.9, -0.4), 0.9)], width=256, height=256)
    v = np.ascontiguousarray(scale(data))
    params = dict(spp=32, max_depth=6, seed=11)
    sc = api.Scene(data).upload(gpu)
    sc.dynamic_lights = True
    sc.refit(v, normals=data.normals)
    sc.refit(data.vertices, normals=data.normals)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    cam = data.camera
    f0 = torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda")
    f1 = torch.zeros_like(f0)
    d_v, d_n = torch.from_numpy(v).cuda(), torch.from_numpy(np.ascontiguousarray(data.normals)).cuda()
    torch.cuda.synchronize()
    sc.render_device(f0.data_ptr(), None, stream=sa.cuda_stream, **params)
    sc.refit_device(d_v.data_ptr(), d_n.data_ptr(), stream=sb.cuda_stream)
    sc.render_device(f1.data_ptr(), None, stream=sa.cuda_stream, **params)
    torch.cuda.synchronize()
    assert sc.light_update_info()["updates"] == 3
    old, new = api.Scene(data).upload(gpu), api.Scene(with_vertices(data, v)).upload(gpu)
    want0, want1 = old.render(**params), new.render(**params)
    assert np.abs(want0 - want1).max() > 1e-3  # the motion is visible
    compare_images(f0.cpu().numpy(), want0, max_bad=0)
    compare_images(f1.cpu().numpy(), want1, max_bad=0)
    for s in (sc, old, new):
        s.close()
