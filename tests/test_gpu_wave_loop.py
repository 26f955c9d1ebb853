"""The wave loop of the fp64 one-pass render kernels (-m gpu): round control from two lane masks, the leaf loop that
alternates two register sets for the prefetched plane, the inside test without NaN quieting.  None of them may change a
decision, so everything here is an equality with what the commit before them rendered:

  * frames, rays_closest and rays_shadow of a 40 x 32 scene at spp 1 / 2 / 7, with and without pixel jitter, depth 20, are
    those of tests/golden/wave_loop_parent.npz bit for bit (rendered on an MI355X by the commit named in
    tests/golden/wave_loop_parent.txt) — from the shipped library, and from the dev-hooks library at three threshold sets:
    the defaults, KEEP 0 with LEAF_BATCH 1 (a leaf round after every node round, a pass as soon as one lane is idle) and
    CHAIN_MIN 65 (no chain step between rounds: every continuation ray starts in a pass).  The "_items" entries are the
    spp 7 frames dealt as one work item per pixel (sample_chunks=1: the sample turnover inside an item);
  * the same for the CookTorrance permutation, which takes the same wave loop;
  * the other instantiations of both permutations — padded records, shading tables in global memory, both — and the
    ray-batch kernels (prt_ray_color: the RAYS | EXTRA permutations): two frames each, and one batch of rays, against the same
    fixture (which multiply-adds the compiler fuses is decided per instantiation);
  * one counting run: node fetches, triangle tests and tris_full are the fixture's (the counting instantiations stay the
    model tests/test_gpu_traversal_work.py checks).

The scene is built for the leaf loop: its tree holds leaves of 1, 2, 3 and 4 triangles (asserted on the dumped tree), so the
two-at-a-time loop ends after an odd and after an even number of tests; a mirror ball; the quad light in view; and a
zero-area triangle whose edge functions are NaN (n / 0), lying across the view so that camera and bounce rays meet its
plane inside their interval and the inside test sees NaN barycentrics.
"""
import os

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes
from pooraytracer_amd.scenes import Material
from tests import bvh_model as M
from tests.test_gpu_kernel_matrix import PERMS, VALID, _render_counting, variant

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wave_loop_parent.npz")
DEPTH, SEED = 20, 11
SPPS = (1, 2, 7)
EMISSION = (14.0, 13.0, 11.0)
THRESHOLDS = {"defaults": {}, "keep0_leafbatch1": {"KEEP": 0, "LEAF_BATCH": 1}, "chain65": {"CHAIN_MIN": 65}}
HOOKS = ("KEEP", "LEAF_BATCH", "CHAIN_MIN", "CACHED_MIN", "INNER_MIN", "TRI_STRIDE", "NO_LDS")
VARIANTS = {"pad": {"TRI_STRIDE": 128}, "no_lds": {"NO_LDS": 1}, "pad_no_lds": {"TRI_STRIDE": 128, "NO_LDS": 1}}
VARIANT_CASES = ("spp2_jitter", "spp7_plain_items")
RAY_KW = dict(spp=3, max_depth=DEPTH, seed=SEED)
COUNT_KW = dict(spp=2, sample_chunks=1)
WORK_KEYS = ("rays_closest", "rays_shadow", "node_fetches", "tri_tests", "tri_full")


def wave_loop_scene(perm):
    """A closed box, the quad light in view, a mirror ball, a ball whose material selects `perm` ("lean": Lambertian; "ct":
    CookTorrance), a fan of slivers, lone triangles and two stacks of near-coincident triangles (leaves of every size) and one
    zero-area triangle across the view."""
    b = scenes._Builder(f"wave-loop-{perm}")
    white = b.material(Material("White", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    red = b.material(Material("Red", _abi.MAT_LAMBERTIAN, kd=(0.63, 0.065, 0.05)))
    green = b.material(Material("Green", _abi.MAT_LAMBERTIAN, kd=(0.14, 0.45, 0.091)))
    light = b.material(Material("Light", _abi.MAT_DIFFUSE_LIGHT, emission=EMISSION))
    b.mesh("floor", white, *scenes.quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)))
    b.mesh("ceiling", white, *scenes.quad((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)))
    b.mesh("back", white, *scenes.quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)))
    b.mesh("left", red, *scenes.quad((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1)))
    b.mesh("right", green, *scenes.quad((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)))
    b.mesh("front", white, *scenes.quad((1, -1, 1), (-1, -1, 1), (-1, 1, 1), (1, 1, 1)))
    b.mesh("light", light, *scenes.quad((-0.3, 0.995, -0.6), (0.3, 0.995, -0.6), (0.3, 0.995, 0.0), (-0.3, 0.995, 0.0)))
    mirror = b.material(Material("Mirror", _abi.MAT_MIRROR))
    if perm == "ct":
        ball = b.material(Material("GoldAniso", _abi.MAT_COOKTORRANCE, kd=(0.8, 0.6, 0.2), eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2),
                                   alpha_x=0.08, alpha_y=0.5))
    else:
        ball = b.material(Material("Ball", _abi.MAT_LAMBERTIAN, kd=(0.5, 0.5, 0.8)))
    v, uv, n = scenes.icosphere(1, radius=0.3, center=(-0.45, 0.1, -0.45))
    b.mesh("mirror-ball", mirror, v, uv, n)
    v, uv, n = scenes.icosphere(1, radius=0.27, center=(0.5, -0.05, -0.5))
    b.mesh("ball", ball, v, uv, n)
    # a fan of 7 slivers around one apex, three lone triangles far from each other, a strip of 5: leaves the SAH cannot fill evenly
    apex = np.array([0.0, -0.35, -0.2])
    ring = [apex + 0.28 * np.array([np.cos(a), 0.35 * np.sin(2 * a), np.sin(a)]) for a in np.linspace(0.0, 1.9 * np.pi, 8)]
    b.mesh("fan", green, np.array([[apex, ring[i], ring[i + 1]] for i in range(7)]))
    lone = [[(-0.9, 0.6, -0.9), (-0.7, 0.6, -0.9), (-0.8, 0.8, -0.85)], [(0.7, 0.5, -0.9), (0.9, 0.5, -0.9), (0.8, 0.7, -0.85)],
            [(0.0, -0.95, 0.5), (0.2, -0.95, 0.5), (0.1, -0.95, 0.3)]]
    b.mesh("lone", red, np.array(lone, dtype=np.float64))
    xs = np.linspace(-0.6, 0.15, 6)
    strip = [[(xs[i], 0.55, -0.8), (xs[i + 1], 0.55, -0.8), (0.5 * (xs[i] + xs[i + 1]), 0.7 + 0.02 * i, -0.78)] for i in range(5)]
    b.mesh("strip", white, np.array(strip, dtype=np.float64))
    # three and four triangles of one outline, 2e-3 apart along their normal: no split of them is cheaper than one leaf
    spots = ((3, (-0.1, -0.6, -0.55)), (4, (0.35, 0.45, -0.7)), (3, (0.0, 0.5, -0.92)), (4, (0.6, -0.6, 0.0)), (3, (-0.75, 0.3, -0.1)),
             (4, (-0.3, 0.75, -0.5)))
    for i, (k, (cx, cy, cz)) in enumerate(spots):
        stack = [[(cx - 0.2, cy - 0.12, cz + 0.002 * j), (cx + 0.2, cy - 0.12, cz + 0.002 * j), (cx, cy + 0.2, cz + 0.002 * j)] for j in range(k)]
        b.mesh(f"stack{i}", red if k == 3 else green, np.array(stack, dtype=np.float64))
    # zero-area: two equal vertices.  Its normal falls back to the vertex normals (+z), its plane is z = 0.1, its edge functions
    # are n / 0 = NaN; its box spans the middle of the view.
    deg = np.array([[[-0.5, -0.4, 0.1], [-0.5, -0.4, 0.1], [0.5, 0.6, 0.1]]], dtype=np.float64)
    b.mesh("degenerate", white, deg, None, np.array([[[0.0, 0.0, 1.0]] * 3]))
    return b.build(scenes.Camera(40, 32, 60.0, eye=(0.0173, 0.0091, 0.95), look_at=(0.0, 0.4, -0.3)))


_DATA = {}


def _data(perm):
    if perm not in _DATA:
        _DATA[perm] = wave_loop_scene(perm)
    return _DATA[perm]


def _set(monkeypatch, setting):
    for k in HOOKS:
        monkeypatch.delenv(f"PRT_TUNE_{k}", raising=False)
    for k, v in setting.items():
        monkeypatch.setenv(f"PRT_TUNE_{k}", str(v))


def cases():
    """(fixture key, render arguments) of every frame of the fixture."""
    out = []
    for spp in SPPS:
        for jitter in (False, True):
            out.append((f"spp{spp}_{'jitter' if jitter else 'plain'}", dict(spp=spp, pixel_jitter=jitter)))
    out.append(("spp7_plain_items", dict(spp=7, pixel_jitter=False, sample_chunks=1)))
    out.append(("spp7_jitter_items", dict(spp=7, pixel_jitter=True, sample_chunks=1)))
    return out


def render_case(sc, kw):
    img = sc.render(max_depth=DEPTH, seed=SEED, **kw)
    cnt = sc.counters()
    return np.ascontiguousarray(img).view(np.uint64), np.array([cnt["rays_closest"], cnt["rays_shadow"], cnt["samples"]], dtype=np.uint64)


def ray_case(sc):
    """RayColor of 1,500 rays shot through the scene's box: the (n, 3) means as bits, and the ray counters."""
    lo, hi = sc.data.bounds()
    rays = scenes.random_rays(1500, lo, hi, seed=77)
    out = sc.ray_color(rays, **RAY_KW)
    cnt = sc.counters()
    return np.ascontiguousarray(out).view(np.uint64), np.array([cnt["rays_closest"], cnt["rays_shadow"]], dtype=np.uint64)


def counting_case(sc):
    img, cnt = _render_counting(sc, max_depth=DEPTH, seed=SEED, **COUNT_KW)
    return np.ascontiguousarray(img).view(np.uint64), np.array([cnt[k] for k in WORK_KEYS], dtype=np.uint64)


def _check_frames(sc, perm, g, where):
    for key, kw in cases():
        bits, counters = render_case(sc, kw)
        bad = int((bits != g[f"{perm}_{key}_bits"]).any(-1).sum())
        assert bad == 0, (perm, where, key, f"{bad} pixels differ from the parent's frame")
        assert counters.tolist() == g[f"{perm}_{key}_counters"].tolist(), (perm, where, key)
    assert variant(sc) & VALID and variant(sc) & _abi.VARIANT_PERM_MASK == PERMS[perm]


@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_the_scene_is_what_the_checks_need(gpu, dev_lib, monkeypatch, tmp_path, perm):
    """Leaves of every size from 1 to PRT_LEAF_MAX in the tree the kernels walk, NaN edge functions on the zero-area triangle
    (the fixture's frames are finite all the same), and a pixel that sees the emitter directly."""
    data = _data(perm)
    path = str(tmp_path / "tree.bin")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    sc = api.Scene(data).upload(gpu)
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    tree = M.read_dump(path)
    refs = tree.nodes["ref"]
    used = (refs < 0) & (refs != M.UNUSED)
    _, cnt = M.decode_leaf(refs[used])
    sizes = {k: int((cnt == k).sum()) for k in range(1, M.LEAF_MAX + 1)}
    print(f"\n{perm}: {tree.n_nodes} nodes, leaves by size {sizes}")
    assert all(sizes.values()), sizes
    deg = data.vertices[int(data.mesh_first_tri[data.mesh_names.index("degenerate")])]
    assert not np.cross(deg[1] - deg[0], deg[2] - deg[0]).any()
    g = np.load(GOLDEN)
    frame = g[f"{perm}_spp1_plain_bits"].view(np.float64)
    assert np.isfinite(frame).all()
    assert (frame == np.array(EMISSION)).all(-1).any(), "no pixel looks straight at the light"
    sc.close()


@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_frames_and_ray_counts_are_the_parents(gpu, perm):
    """The shipped library."""
    g = np.load(GOLDEN)
    sc = api.Scene(_data(perm)).upload(gpu)
    _check_frames(sc, perm, g, "shipped")
    sc.close()


@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_frames_and_ray_counts_are_the_parents_at_every_threshold_set(gpu, dev_lib, monkeypatch, perm, thresholds):
    g = np.load(GOLDEN)
    _set(monkeypatch, THRESHOLDS[thresholds])
    sc = api.Scene(_data(perm)).upload(gpu)
    _check_frames(sc, perm, g, thresholds)
    sc.close()


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_other_instantiations_render_the_parents_frames(gpu, dev_lib, monkeypatch, perm, name):
    g = np.load(GOLDEN)
    _set(monkeypatch, VARIANTS[name])
    sc = api.Scene(_data(perm)).upload(gpu)
    for key, kw in cases():
        if key in VARIANT_CASES:
            bits, counters = render_case(sc, kw)
            assert np.array_equal(bits, g[f"{perm}_{name}_{key}_bits"]), (perm, name, key)
            assert counters.tolist() == g[f"{perm}_{name}_{key}_counters"].tolist(), (perm, name, key)
    v = variant(sc)
    assert bool(v & _abi.VARIANT_PAD) == ("pad" in name) and (not v & _abi.VARIANT_LLDS or "no_lds" not in name), (name, v)
    sc.close()


@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_ray_batches_get_the_parents_radiance(gpu, perm):
    g = np.load(GOLDEN)
    sc = api.Scene(_data(perm)).upload(gpu)
    bits, counters = ray_case(sc)
    assert np.array_equal(bits, g[f"{perm}_rays_bits"]) and counters.tolist() == g[f"{perm}_rays_counters"].tolist()
    assert counters[0] > 1500 and counters[1] > 0
    sc.close()


@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_counting_run_does_the_parents_work(gpu, perm):
    """Node fetches, triangle tests and tris_full of one counting run (and its frame and ray counts) are the fixture's."""
    g = np.load(GOLDEN)
    sc = api.Scene(_data(perm)).upload(gpu)
    bits, work = counting_case(sc)
    assert dict(zip(WORK_KEYS, work.tolist())) == dict(zip(WORK_KEYS, g[f"{perm}_counting_work"].tolist()))
    assert np.array_equal(bits, g[f"{perm}_counting_bits"])
    assert work[2] > 0 and work[3] > work[4] > 0
    sc.close()
