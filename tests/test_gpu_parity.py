"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the
same seeded inputs, against the committed golden fixtures, and through size-independent properties.

Tolerances (fp64 arithmetic on both sides; differences come only from FMA contraction / libm ulps):
  * closest hit: same primitive (except exact-t ties), |dt| <= 1e-12 * max(1,t)
  * light sampling: bit-exact triangle choice, positions to 1e-13
  * rendered image with identical per-sample RNG keys: per-channel |d| <= 1e-9 * max(1,|x|) for every
    pixel.  compare_images allows NO pixel beyond it on images below 10^5 pixels and two on whole frames: the one event known
    to take the other side of a branch is a random draw of exactly 0 (2^-31 per draw, its own test below); nothing else has
    been seen to differ on whole frames or on 3,000 random scenes.
"""
import json
import os

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, scenes
from tests import frame_model

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def compare_hits(g, o):
    assert np.array_equal(g["prim"] >= 0, o["prim"] >= 0)
    hit = o["prim"] >= 0
    # |dt| <= 1e-12 * max(1, t): t = (D - n.o) / (n.d) cancels, so a hit a millimetre from the origin of a
    # ray that starts metres from the triangle's plane carries the plane's absolute rounding, not t's relative one
    assert (np.abs(g["t"][hit] - o["t"][hit]) <= 1e-12 * np.maximum(1.0, o["t"][hit])).all()
    same = g["prim"] == o["prim"]
    # a different primitive is only acceptable on an exact tie in t (shared edge / coplanar)
    assert (g["t"][~same] == o["t"][~same]).all()
    both = hit & same
    assert np.allclose(g["alpha"][both], o["alpha"][both], atol=1e-10)
    assert np.allclose(g["beta"][both], o["beta"][both], atol=1e-10)
    assert np.array_equal(g["front"][both], o["front"][both])
    assert np.isinf(g["t"][~hit]).all()


def compare_images(gpu_img, cpu_img, max_bad=None):
    """Every pixel within 1e-9 per channel.  `max_bad` is an ABSOLUTE pixel count: 0 on anything below 10^5 pixels, 2 on whole
    frames (the one event known to take the other side of a branch is a random draw of exactly 0, 2^-31 per draw: about one
    pixel per 10^9 samples — DESIGN.md §3; nothing else has been seen to differ on whole frames or on 3,000 random scenes)."""
    tol = 1e-9 * np.maximum(1.0, np.abs(cpu_img))
    bad = (np.abs(gpu_img - cpu_img) > tol).any(axis=-1)
    if max_bad is None:
        max_bad = 0 if bad.size < 100_000 else 2
    assert bad.sum() <= max_bad, f"{bad.sum()} of {bad.size} pixels differ: {np.argwhere(bad)[:8].tolist()}"
    assert np.allclose(gpu_img.mean(axis=(0, 1)), cpu_img.mean(axis=(0, 1)), rtol=2e-3)
    if bad.sum() == 0:
        assert np.allclose(gpu_img.mean(axis=(0, 1)), cpu_img.mean(axis=(0, 1)), rtol=1e-9)
    return int(bad.sum())


def assert_ray_counts(gpu_cnt, cpu_cnt):
    """The GPU never traces a ray whose result the reference discards (the peek at the depth limit,
    Camera.cpp:187 with depth-1 < 0; shadow rays failing the n.wi / front-face tests, Camera.cpp:150-154;
    continuations with zero throughput), so its counts are bounded by the oracle's and close to them."""
    assert gpu_cnt["rays_closest"] <= cpu_cnt["rays_closest"]
    assert gpu_cnt["rays_closest"] >= 0.9 * cpu_cnt["rays_closest"]
    assert gpu_cnt["rays_shadow"] <= cpu_cnt["rays_shadow"]
    assert gpu_cnt["rays_shadow"] >= 0.2 * cpu_cnt["rays_shadow"]


@pytest.mark.parametrize("name", ["tiny_cornell", "mixed"])
def test_golden_hits_and_image(gpu, name):
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    meta = json.loads(str(g["meta"]))
    data = scenes.tiny_scene() if name == "tiny_cornell" else scenes.mixed_materials()
    sc = api.Scene(data).upload(gpu)
    assert np.array_equal(sc.light_order(), g["light_order"])
    rays = g["rays"].view(_abi.RAY_DTYPE).reshape(-1)
    h = sc.trace_closest(rays)
    gold = np.zeros(rays.shape[0], dtype=_abi.HIT_DTYPE)
    for k in ("t", "prim", "alpha", "beta", "front"):
        gold[k] = g["hit_" + k]
    compare_hits(h, gold)
    img = sc.render(spp=meta["spp"], max_depth=meta["max_depth"], seed=meta["seed"])
    compare_images(img, g["image"])
    cnt = sc.counters()
    assert cnt["samples"] == data.camera.width * data.camera.height * meta["spp"]
    assert_ray_counts(cnt, meta["counters"])


def test_random_rays_vs_oracle_cornell(gpu):
    data = scenes.cornell_box(ball_subdiv=3, width=64, height=64)
    lo, hi = data.bounds()
    rays = scenes.random_rays(50000, lo - 0.5, hi + 0.5, seed=11)
    o = oracle.Oracle(data).trace_closest(rays)
    sc = api.Scene(data).upload(gpu)
    compare_hits(sc.trace_closest(rays), o)
    # counting instantiation returns the same hits and non-zero work counters
    h2 = sc.trace_closest(rays, count_work=True)
    compare_hits(h2, o)
    cnt = sc.counters()
    assert cnt["rays_closest"] == 50000 and cnt["node_fetches"] > 50000 and cnt["tri_tests"] > 0


def test_edge_cases_rays(gpu):
    """Axis-aligned directions (zero components -> inf reciprocals), rays starting on surfaces,
    degenerate intervals, empty batch, single-triangle and empty scenes."""
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    o = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0.1, -1, 0.3], [0, 0, 3], [0.3, 0.2, 0.5]], dtype=np.float64)
    d = np.array([[0, -1, 0], [1, 0, 0], [0, 0, -1], [0, 1, 0], [0, 0, 1], [0, 0, -1e-3]], dtype=np.float64)
    rays = np.zeros(6, dtype=_abi.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmin"], rays["tmax"] = o, d, 1e-4, np.inf
    compare_hits(sc.trace_closest(rays), orc.trace_closest(rays))
    rays["tmax"] = 0.5  # clipped interval
    compare_hits(sc.trace_closest(rays), orc.trace_closest(rays))
    assert sc.trace_closest(rays[:0]).shape[0] == 0
    # one triangle
    from tests.test_oracle import one_triangle
    one = one_triangle()
    s1 = api.Scene(one).upload(gpu)
    lo, hi = one.bounds()
    r = scenes.random_rays(2000, lo - 1, hi + 1, seed=5)
    compare_hits(s1.trace_closest(r), oracle.Oracle(one).trace_closest(r))


def test_light_sampling_bit_exact(gpu):
    for data in (scenes.tiny_scene(), scenes.veach_mis(64, 36, light_subdiv=2, plate_cells=2)):
        sc = api.Scene(data).upload(gpu)
        orc = oracle.Oracle(data)
        assert np.array_equal(sc.light_order(), orc.light_order())
        rng = np.random.default_rng(3)
        org = rng.uniform(-1, 1, size=(20000, 3))
        a, b = sc.sample_lights(org, seed=42), orc.sample_lights(org, seed=42)
        assert np.array_equal(a["prim"], b["prim"])
        assert np.array_equal(a["front"], b["front"])
        assert np.allclose(a["position"], b["position"], rtol=0, atol=1e-13)
        assert np.allclose(a["normal"], b["normal"], rtol=0, atol=1e-15)
        assert np.array_equal(a["pdf"], b["pdf"])


@pytest.mark.parametrize("scene_fn,spp,depth", [
    (lambda: scenes.cornell_box(ball_subdiv=2, width=64, height=64), 8, 10),
    (lambda: scenes.mixed_materials(40, 40), 12, 12),
    (lambda: scenes.veach_mis(96, 54, light_subdiv=2, plate_cells=2), 8, 20),
    (lambda: scenes.bathroom(64, 36, detail=0.12), 4, 12),
])
def test_render_vs_oracle(gpu, scene_fn, spp, depth):
    data = scene_fn()
    cpu, ccnt = oracle.Oracle(data).render(spp=spp, max_depth=depth, seed=3, nthreads=8)
    sc = api.Scene(data).upload(gpu)
    img = sc.render(spp=spp, max_depth=depth, seed=3)
    compare_images(img, cpu)
    cnt = sc.counters()
    assert cnt["samples"] == ccnt["samples"]
    assert_ray_counts(cnt, ccnt)


def test_exact_tie_rays_documented(gpu):
    """Symmetric camera: pixel-centre rays on the image diagonals hit the box edges exactly, i.e. two
    triangles of different materials at bit-identical t.  The winner of such a tie depends on BVH test
    order (reference included), so those pixels — and only those — may differ from the oracle."""
    data = scenes.cornell_box(ball_subdiv=1, width=64, height=64, symmetric_camera=True)
    cpu, _ = oracle.Oracle(data).render(spp=4, max_depth=6, seed=2)
    img = api.Scene(data).upload(gpu).render(spp=4, max_depth=6, seed=2)
    tol = 1e-9 * np.maximum(1.0, np.abs(cpu))
    bad = (np.abs(img - cpu) > tol).any(axis=-1)
    jj, ii = np.nonzero(bad)
    assert ((ii == jj) | (ii == 63 - jj)).all()


def test_render_options(gpu):
    """bSampleLights off, non-black background, RR 1.0, depth 0, chunked sample partitions."""
    data = scenes.mixed_materials(32, 32)
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    for kw in (dict(spp=4, max_depth=5, sample_lights=False, background=(0.2, 0.3, 0.4)),
               dict(spp=3, max_depth=0), dict(spp=4, max_depth=6, rr=1.0), dict(spp=5, max_depth=4, rr=0.5, seed=99),
               dict(spp=6, max_depth=5, pixel_jitter=True, seed=5)):
        cpu, _ = orc.render(**kw)
        compare_images(sc.render(**kw), cpu)
    # chunked partial sums only change the summation order (<= 1e-15 relative)
    a = sc.render(spp=16, max_depth=6, sample_chunks=1)
    b = sc.render(spp=16, max_depth=6, sample_chunks=4)
    assert np.allclose(a, b, rtol=1e-13, atol=1e-15)
    # determinism: bitwise identical across runs
    assert np.array_equal(b, sc.render(spp=16, max_depth=6, sample_chunks=4))
    # the automatic item schedule (a share-dependent geometric tail, <= 64 chunks) covers every sample exactly
    # once at any spp: very high spp on few pixels, tile shares that leave a rank a single tile, spp = 1
    small = scenes.Camera(24, 16, data.camera.fovy, data.camera.eye, data.camera.look_at)
    for kw in (dict(spp=4100, max_depth=1), dict(spp=333, max_depth=2, rank=1, nranks=3, tile_size=8), dict(spp=1, max_depth=3)):
        one = sc.render(camera=small, sample_chunks=1, **kw)
        auto = sc.render(camera=small, **kw)
        assert np.allclose(auto, one, rtol=1e-12, atol=1e-15), kw


def test_tile_sharding_sums_to_full_image(gpu):
    """Multi-GPU partition (one rank after another on this GPU): disjoint tiles, zero elsewhere,
    sum over ranks bit-identical to the single-rank image."""
    data = scenes.cornell_box(ball_subdiv=1, width=80, height=56)  # not a multiple of the tile size
    sc = api.Scene(data).upload(gpu)
    full = sc.render(spp=4, max_depth=6, tile_size=16, sample_chunks=1)
    for nranks in (2, 3, 8):
        parts = [sc.render(spp=4, max_depth=6, tile_size=16, rank=r, nranks=nranks, sample_chunks=1) for r in range(nranks)]
        nz = np.stack([(p != 0).any(-1) for p in parts])
        assert (nz.sum(0) <= 1).all()
        assert np.array_equal(np.sum(parts, axis=0), full)


def test_f32_output_and_tonemap(gpu):
    import torch
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(gpu)
    img64, img32 = sc.render(spp=4, max_depth=5, f32=True)
    assert np.array_equal(img32, img64.astype(np.float32))
    t = torch.from_numpy(img32).cuda()
    t[0, 0, 0] = float("nan")
    u8 = torch.zeros(t.shape, dtype=torch.uint8, device="cuda")
    sc.tonemap_srgb8(t.data_ptr(), 64, 64, u8.data_ptr())
    torch.cuda.synchronize()
    # the bytes of the fp64 model exactly; only where sv * 255 lies within 1e-9 of an integer may the device's pow round over
    ref, near = frame_model.srgb8(t.cpu().numpy())
    off = u8.cpu().numpy() != ref
    assert not (off & ~near).any(), np.argwhere(off & ~near)[:8].tolist()


def test_full_size_properties(gpu):
    """BASELINE config sizes via size-independent properties (no oracle at this size):
    1024x1024 cornell, spp 2: determinism, sample count, energy bound, light pixels exact."""
    data = scenes.cornell_box()
    sc = api.Scene(data).upload(gpu)
    a = sc.render(spp=2, max_depth=20)
    cnt = sc.counters()
    assert cnt["samples"] == 1024 * 1024 * 2
    assert np.isfinite(a).all() and (a >= 0).all()
    assert np.array_equal(a, sc.render(spp=2, max_depth=20))
    # pixels looking straight at the light return exactly its radiance
    lit = (a == np.array([17.0, 12.0, 4.0])).all(-1)
    assert lit.sum() > 1000
    # a row band rendered by the oracle matches
    cpu, _ = oracle.Oracle(data).render(spp=2, max_depth=20, rows=(500, 504), nthreads=4)
    compare_images(a[500:504], cpu[500:504])


def test_closest_hit_optimality_large_soup(gpu):
    """Size-independent properties of K1 on a BVH far beyond the oracle's reach (2M random triangles,
    deep tree): (1) every reported hit lies on its triangle: o + t d == v0 + alpha e0 + beta e1 with
    valid barycentrics; (2) closest-ness: re-tracing with tmax just below t finds nothing on the same
    primitive and anything it finds is strictly nearer than t is impossible -> must be a miss;
    (3) a brute-force check of a ray subset against ALL triangles with the reference formulas."""
    data = scenes.triangle_soup(2_000_000, seed=9, with_light=False)
    sc = api.Scene(data).upload(gpu)
    assert sc.counters()["bvh_depth"] <= 30
    lo, hi = data.bounds()
    rays = scenes.random_rays(200_000, lo, hi, seed=21)
    h = sc.trace_closest(rays)
    hit = h["prim"] >= 0
    assert hit.mean() > 0.5
    v = data.vertices[h["prim"][hit]]
    p_ray = rays["o"][hit] + rays["d"][hit] * h["t"][hit, None]
    p_tri = v[:, 0] + h["alpha"][hit, None] * (v[:, 1] - v[:, 0]) + h["beta"][hit, None] * (v[:, 2] - v[:, 0])
    assert np.abs(p_ray - p_tri).max() < 1e-10
    assert (h["alpha"][hit] >= 0).all() and (h["beta"][hit] >= 0).all() and (h["alpha"][hit] + h["beta"][hit] <= 1 + 1e-15).all()
    assert (h["t"][hit] >= 1e-4).all()
    # closest-ness: nothing in [tmin, t*(1-1e-9)]
    r2 = rays[hit].copy()
    r2["tmax"] = h["t"][hit] * (1 - 1e-9)
    assert (sc.trace_closest(r2)["prim"] == -1).all()
    # brute force for a few rays (reference formulas, Triangle.cpp:54-83)
    V = data.vertices
    e0, e1 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    n = np.cross(e0, e1)
    nn = n / np.linalg.norm(n, axis=1, keepdims=True)
    D = (nn * V[:, 0]).sum(1)
    w = n / (n * n).sum(1, keepdims=True)
    for i in range(0, 200_000, 20_000):
        oo, dd = rays["o"][i], rays["d"][i]
        den = nn @ dd
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (D - nn @ oo) / den
        v0p = oo + dd * t[:, None] - V[:, 0]
        al = (w * np.cross(v0p, e1)).sum(1)
        be = (w * np.cross(e0, v0p)).sum(1)
        ok = (np.abs(den) >= 1e-8) & (t >= 1e-4) & (al >= 0) & (be >= 0) & (al + be <= 1)
        if ok.any():
            tt = np.where(ok, t, np.inf)
            assert h["prim"][i] == int(np.argmin(tt)) or h["t"][i] == tt.min()
            assert abs(h["t"][i] - tt.min()) <= 1e-12 * max(1.0, tt.min())
        else:
            assert h["prim"][i] == -1


@pytest.mark.parametrize("name", ["veach", "bathroom"])
def test_full_size_other_configs(gpu, name):
    """BASELINE configs 3/4 at their real resolution (1280x720) and depth, spp 2: determinism,
    counts, finiteness, and oracle parity on a 4-row band."""
    data = scenes.veach_mis() if name == "veach" else scenes.bathroom()
    depth = 100 if name == "veach" else 50
    sc = api.Scene(data).upload(gpu)
    a = sc.render(spp=2, max_depth=depth)
    cnt = sc.counters()
    assert cnt["samples"] == 1280 * 720 * 2
    assert np.isfinite(a).all() and (a >= 0).all()
    assert np.array_equal(a, sc.render(spp=2, max_depth=depth))
    cpu, _ = oracle.Oracle(data).render(spp=2, max_depth=depth, rows=(400, 404), nthreads=8)
    compare_images(a[400:404], cpu[400:404])


def _torture_scene():
    """Degenerate inputs in one scene: a zero-area triangle (NaN normal -> vertex-normal / +z fallback,
    Triangle.cpp:21-29), a triangle with identical texcoords (NaN tangent fallback, :39-46), a 1-channel
    texture (grey, no sRGB decode, Texture.cpp:61-63), a missing texture (cyan, Texture.cpp:24), an
    Empty absorber and a Debug emitter."""
    b = scenes._Builder("torture")
    b.textures.append((np.arange(16 * 16, dtype=np.uint8).reshape(16, 16) * 1).copy())   # 1 channel
    b.textures.append(np.zeros((0, 0, 3), dtype=np.uint8))                                # no data -> (0,1,1)
    grey = b.material(scenes.Material("Wood", _abi.MAT_LAMBERTIAN, kd=(0.5, 0.5, 0.5), texture=0))
    cyan = b.material(scenes.Material("WoodFloor", _abi.MAT_LAMBERTIAN, kd=(0.5, 0.5, 0.5), texture=1))
    white = b.material(scenes.Material("DiffuseWhite", _abi.MAT_LAMBERTIAN, kd=(0.8, 0.8, 0.8)))
    light = b.material(scenes.Material("Light", _abi.MAT_DIFFUSE_LIGHT, emission=(9.0, 9.0, 9.0)))
    empty = b.material(scenes.Material("quad1", _abi.MAT_EMPTY))
    debug = b.material(scenes.Material("Debug", _abi.MAT_DEBUG, kd=(0.2, 0.1, 0.4)))
    b.mesh("floor", grey, *scenes.quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)))
    b.mesh("back", cyan, *scenes.quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)))
    b.mesh("left", white, *scenes.quad((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1)))
    b.mesh("light", light, *scenes.quad((-0.4, 0.99, -0.4), (0.4, 0.99, -0.4), (0.4, 0.99, 0.4), (-0.4, 0.99, 0.4)))
    b.mesh("absorber", empty, *scenes.quad((0.2, -0.99, 0.0), (0.6, -0.99, 0.0), (0.6, -0.99, 0.4), (0.2, -0.99, 0.4)))
    b.mesh("debug", debug, *scenes.quad((0.95, -0.5, -0.5), (0.95, -0.5, 0.5), (0.95, 0.5, 0.5), (0.95, 0.5, -0.5)))
    # degenerate: zero-area triangle with a usable vertex normal, and one with all-equal UVs
    deg_v = np.array([[[0, 0, 0], [0, 0, 0], [0.5, 0.5, 0]], [[-0.5, -0.9, 0.2], [0.0, -0.9, 0.2], [-0.25, -0.5, 0.2]]], dtype=np.float64)
    deg_uv = np.array([[[0, 0], [1, 0], [0, 1]], [[0.3, 0.3], [0.3, 0.3], [0.3, 0.3]]], dtype=np.float64)
    deg_n = np.array([[[0, 0, 1]] * 3, [[0, 0, 0]] * 3], dtype=np.float64)
    b.mesh("degenerate", white, deg_v, deg_uv, deg_n)
    return b.build(scenes.Camera(40, 32, 70.0, (0.03, 0.05, 1.6), (0.0, -0.2, 0.0)))


def test_degenerate_inputs_and_textures(gpu):
    data = _torture_scene()
    cpu, _ = oracle.Oracle(data).render(spp=6, max_depth=6, seed=4)
    assert np.isfinite(cpu).all()
    sc = api.Scene(data).upload(gpu)
    compare_images(sc.render(spp=6, max_depth=6, seed=4), cpu)
    lo, hi = data.bounds()
    rays = scenes.random_rays(20000, lo - 0.2, hi + 0.2, seed=8)
    compare_hits(sc.trace_closest(rays), oracle.Oracle(data).trace_closest(rays))


def test_empty_and_lightless_scenes(gpu):
    # no triangles at all: every pixel is the background, every ray misses
    b = scenes._Builder("empty")
    b.material(scenes.Material("DiffuseWhite", _abi.MAT_LAMBERTIAN, kd=(0.5, 0.5, 0.5)))
    empty = scenes.SceneData("empty", np.zeros((0, 3, 3)), np.zeros((0, 3, 2)), np.zeros((0, 3, 3)), np.array([0], dtype=np.uint64),
                             np.zeros(0, dtype=np.int32), [], b.materials, scenes.Camera(16, 8, 60.0, (0, 0, 1), (0, 0, 0)))
    sc = api.Scene(empty).upload(gpu)
    img = sc.render(spp=3, max_depth=4, background=(0.25, 0.5, 0.75))
    assert np.allclose(img, [0.25, 0.5, 0.75], rtol=1e-15)
    h = sc.trace_closest(scenes.random_rays(100, (-1, -1, -1), (1, 1, 1)))
    assert (h["prim"] == -1).all() and np.isinf(h["t"]).all()
    # geometry but no emissive mesh, bSampleLights on: NEE is skipped, only the background lights the scene
    from tests.test_oracle import one_triangle
    one = one_triangle()
    cpu, _ = oracle.Oracle(one).render(spp=8, max_depth=3, background=(0.3, 0.3, 0.3), sample_lights=False)
    compare_images(api.Scene(one).upload(gpu).render(spp=8, max_depth=3, background=(0.3, 0.3, 0.3), sample_lights=False), cpu)
    cpu2, _ = oracle.Oracle(one).render(spp=8, max_depth=3, background=(0.3, 0.3, 0.3), sample_lights=True)
    compare_images(api.Scene(one).upload(gpu).render(spp=8, max_depth=3, background=(0.3, 0.3, 0.3), sample_lights=True), cpu2)


@pytest.mark.gpu
def test_update_vertices_matches_fresh_scene(gpu):
    """Moving geometry: prt_scene_update_vertices (triangle precompute + light tree on the host, BVH rebuilt on the
    GPU) must leave the scene exactly as if it had been created from the new positions."""
    import copy
    data = scenes.cornell_box(ball_subdiv=3, width=40, height=40)
    sc = api.Scene(data).upload(gpu)
    first = sc.render(spp=3, max_depth=5, seed=4)
    moved = copy.copy(data)
    v = data.vertices.copy()
    ball = slice(int(data.mesh_first_tri[-2]), int(data.mesh_first_tri[-1]))  # last mesh = the tessellated ball
    v[ball] = v[ball] * 0.8 + np.array([0.15, 0.1, -0.2])
    lights = np.arange(int(data.mesh_first_tri[-3]), int(data.mesh_first_tri[-2]))
    v[lights] = v[lights] * np.array([1.3, 1.0, 0.7])                          # the light changes area as well
    moved.vertices = v
    sc.update_vertices(v)
    assert sc.bvh_info()["built_on_device"] == 1
    fresh = api.Scene(moved).upload(gpu)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    rays = scenes.random_rays(100_000, lo, hi, seed=23)
    a, b = sc.trace_closest(rays), fresh.trace_closest(rays)
    assert np.array_equal(a["t"], b["t"]) and np.array_equal(a["prim"], b["prim"])
    org = np.random.default_rng(1).uniform(-0.9, 0.9, size=(5000, 3))
    la, lb = sc.sample_lights(org, seed=7), fresh.sample_lights(org, seed=7)
    for f in ("prim", "position", "normal", "pdf", "front"):
        assert np.array_equal(la[f], lb[f]), f
    img, ref = sc.render(spp=3, max_depth=5, seed=4), fresh.render(spp=3, max_depth=5, seed=4)
    assert np.array_equal(img, ref) and not np.array_equal(img, first)
    cpu, _ = oracle.Oracle(moved).render(spp=3, max_depth=5, seed=4)
    compare_images(img, cpu)


@pytest.mark.gpu
def test_update_vertices_rebuilds_the_light_tables(gpu):
    """Moving EMISSIVE geometry of a scene whose light pick goes through the O(1) tables (veach-mis: four spheres, 6,400 light
    triangles): areas, CDF order, thresholds and buckets all change with the vertices; the picks after
    prt_scene_update_vertices are the oracle's picks for the new positions, bit for bit."""
    import copy
    data = scenes.veach_mis(width=64, height=36)
    sc = api.Scene(data).upload(gpu)
    assert sc.bvh_info()["lds_light_nodes"] < 64  # (tables: only the few nodes above them are staged)
    v = data.vertices.copy()
    emissive = [m for m in range(len(data.mesh_material)) if data.materials[int(data.mesh_material[m])].type == _abi.MAT_DIFFUSE_LIGHT]
    assert len(emissive) >= 2
    for k, m in enumerate(emissive):
        sl = slice(int(data.mesh_first_tri[m]), int(data.mesh_first_tri[m + 1]))
        c = v[sl].reshape(-1, 3).mean(0)
        v[sl] = (v[sl] - c) * np.array([1.0 + 0.35 * k, 0.8, 1.1 + 0.1 * k]) + c + np.array([0.02 * k, 0.05, -0.03])
    moved = copy.copy(data)
    moved.vertices = v
    sc.update_vertices(v)
    orc = oracle.Oracle(moved)
    assert np.array_equal(sc.light_order(), orc.light_order())
    org = np.random.default_rng(5).uniform(-3, 3, size=(200_000, 3))
    g, c = sc.sample_lights(org, seed=9), orc.sample_lights(org, seed=9)
    assert np.array_equal(g["prim"], c["prim"]) and np.array_equal(g["front"], c["front"])
    assert np.array_equal(g["pdf"].view(np.uint64), c["pdf"].view(np.uint64))
    assert np.abs(g["position"] - c["position"]).max() <= 1e-13 * max(1.0, np.abs(c["position"]).max())
    img = sc.render(spp=4, max_depth=8, seed=2)
    ref, _ = orc.render(spp=4, max_depth=8, seed=2)
    compare_images(img, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene_fn,nrays", [
    ("tiny", scenes.tiny_scene, 20_000),
    ("cornell", lambda: scenes.cornell_box(ball_subdiv=4, width=48, height=48), 200_000),
    ("bathroom", lambda: scenes.bathroom(64, 36, detail=0.3), 200_000),
    ("soup", lambda: scenes.triangle_soup(300_000), 200_000),
])
def test_device_bvh_build_gives_identical_results(gpu, name, scene_fn, nrays):
    """PRT_SCENE_DEVICE_BVH (tree built on the GPU, bvh_build_gpu.hip) vs the host builder: hits and images do
    not depend on the tree, so they must be bit-identical (the accept/reject arithmetic is the same fp64
    triangle test on the same records); the tree must respect the stack bound and cost about the same to traverse."""
    data = scene_fn()
    host = api.Scene(data).upload(gpu)
    dev = api.Scene(data, device_bvh=True).upload(gpu)
    info = dev.bvh_info()
    n = len(data.vertices)
    assert info["built_on_device"] == 1 and 1 <= info["n_nodes"] < n and info["depth"] <= 30
    lo, hi = data.vertices.reshape(-1, 3).min(0), data.vertices.reshape(-1, 3).max(0)
    rays = scenes.random_rays(nrays, lo, hi, seed=17)
    a, b = host.trace_closest(rays, count_work=True), dev.trace_closest(rays, count_work=True)
    ca, cb = host.counters(), dev.counters()
    assert np.array_equal(a["t"], b["t"])
    same = a["prim"] == b["prim"]
    # exact ties (bathroom: coplanar overlapping faces) go to whichever triangle the tree tests last
    assert same.mean() > (0.99 if name == "bathroom" else 0.9999)
    assert np.array_equal(a["alpha"][same], b["alpha"][same]) and np.array_equal(a["front"][same], b["front"][same])
    # traversal cost of the GPU-built tree stays close to the binned-SAH host tree
    print(f"{name}: nodes/ray host {ca['node_fetches'] / nrays:.1f} device {cb['node_fetches'] / nrays:.1f}; "
          f"tris/ray host {ca['tri_tests'] / nrays:.2f} device {cb['tri_tests'] / nrays:.2f}")
    if n >= 1000:  # a dozen wall-sized triangles have no useful Morton order
        # measured: cornell 1.5x, bathroom 1.6x, soup 1.08x the node visits of the host binned-SAH tree
        assert cb["node_fetches"] <= 2.0 * ca["node_fetches"]
        assert cb["tri_tests"] <= 1.5 * ca["tri_tests"]
    if name in ("tiny", "cornell"):  # no coplanar overlaps => no ties => the images are bit-identical
        ia, ib = host.render(spp=4, max_depth=6, seed=9), dev.render(spp=4, max_depth=6, seed=9)
        assert np.array_equal(ia, ib)
    # determinism of the builder's results across two builds
    dev2 = api.Scene(data, device_bvh=True).upload(gpu)
    assert np.array_equal(dev2.trace_closest(rays)["t"], b["t"])


@pytest.mark.gpu
def test_lds_tables_and_plain_kernels_agree(gpu, dev_lib, monkeypatch):
    """K3 has two kernel families: with the material table / light triangles / top of the light tree staged in LDS
    (default when the materials fit in 8 KB) and without.  Same arithmetic, so the images must be bit-identical —
    on a few-light scene (light triangles staged), a many-light scene (only the top of the tree staged, the rest
    read from global memory) and a scene with more materials than fit (falls back to the plain kernels).  The two
    families are separate compilations of the same source (fused multiply-adds may be formed differently), so
    the comparison uses the image tolerance rather than bit equality."""
    import copy
    few = scenes.mixed_materials(40, 32)
    many = scenes.veach_mis(64, 36, light_subdiv=3, plate_cells=2)          # 5120 light triangles, 13 tree levels
    big = copy.copy(few)
    big.materials = list(few.materials) + [few.materials[0]] * 60             # 60+ materials: > 8 KB
    for data, kw in ((few, dict(spp=6, max_depth=6)), (many, dict(spp=4, max_depth=8)), (big, dict(spp=3, max_depth=4))):
        monkeypatch.delenv("PRT_TUNE_NO_LDS", raising=False)
        a = api.Scene(data).upload(gpu).render(seed=11, **kw)
        monkeypatch.setenv("PRT_TUNE_NO_LDS", "1")
        b = api.Scene(data).upload(gpu).render(seed=11, **kw)
        compare_images(a, b)
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
    monkeypatch.delenv("PRT_TUNE_NO_LDS", raising=False)
    cpu, _ = oracle.Oracle(many).render(spp=4, max_depth=8, seed=11, nthreads=8)
    compare_images(api.Scene(many).upload(gpu).render(spp=4, max_depth=8, seed=11), cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("scale,offset", [(1e-4, (0.0, 0.0, 0.0)), (1.0, (4.0e4, -2.5e4, 1.0e4)), (3.0e3, (1.0e6, 2.0e6, -3.0e6)),
                                          (0.5, (1.0e6, 1.0e6, 1.0e6)), (5.0, (6.0e6, -6.0e6, 6.0e6))])
def test_scaled_and_translated_scene_hits(gpu, scale, offset):
    """The fp32 box tests work on a 16-bit grid over the scene bounds with a per-ray pad proportional to
    |origin| + scene extent: they must stay conservative when the scene is tiny, far from the origin, or large
    and far (fp32 has 24 bits; at 3e6 one ulp is 0.25).  Closest hits against the CPU oracle, which knows no
    boxes' rounding (fp64 slabs)."""
    import copy
    base = scenes.cornell_box(ball_subdiv=3, width=32, height=32)
    data = copy.copy(base)
    off = np.asarray(offset)
    data.vertices = base.vertices * scale + off
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    lo, hi = data.vertices.reshape(-1, 3).min(0), data.vertices.reshape(-1, 3).max(0)
    rays = scenes.random_rays(100_000, lo, hi, seed=31)
    rays["tmin"] = 1e-4 * scale
    b = orc.trace_closest(rays)
    # far from the origin t = (D - n.o)/(n.d) cancels ~|o| digits, and the GPU forms FMAs where the oracle does not:
    # the fp64 results agree to |o| * eps rather than to 1e-12; a box that culled wrongly would instead show up
    # as a miss or as a farther triangle, i.e. a difference of the order of the scene
    mag = float(np.abs(data.vertices).max())
    tol = 64 * np.finfo(np.float64).eps * mag * 1e3 + 1e-12

    def check(g):
        assert np.array_equal(g["prim"] >= 0, b["prim"] >= 0)
        hit = b["prim"] >= 0
        assert np.all(np.abs(g["t"][hit] - b["t"][hit]) <= tol * np.maximum(1.0, b["t"][hit]))
        diff = hit & (g["prim"] != b["prim"])
        assert diff.mean() < 1e-3  # ties within rounding on shared edges only

    check(sc.trace_closest(rays))
    # the device-built tree obeys the same bounds
    check(api.Scene(data, device_bvh=True).upload(gpu).trace_closest(rays))
    # the box test works relative to the grid origin and the builders work on boxes relative to it (prim_boxes): where the
    # scene sits in the world changes neither the tree nor the culling — the far scene costs the node fetches of the near
    # one (round 2, pad proportional to the world coordinate: a unit scene at 1e6 was not culled at all; rounds 2-3, fp32
    # boxes in world coordinates: 16 positions per axis for that scene, 1.5x the fetches)
    if scale < 0.1:  # (a 2e-4 wide scene is mostly the reference's 1e-4 minimum box padding, AABB.cpp:76-82: nothing to cull)
        return
    sc.trace_closest(rays[:20000], count_work=True)
    far = sc.counters()["node_fetches"]
    near = api.Scene(base).upload(gpu)
    r0 = scenes.random_rays(20000, *base.bounds(), seed=31)
    near.trace_closest(r0, count_work=True)
    assert far <= 1.02 * near.counters()["node_fetches"], (far, near.counters()["node_fetches"])
    # ... and so does the tree built on the device (Morton codes and SAH bins on the same relative boxes)
    fd = api.Scene(data, device_bvh=True).upload(gpu)
    fd.trace_closest(rays[:20000], count_work=True)
    nd = api.Scene(base, device_bvh=True).upload(gpu)
    nd.trace_closest(r0, count_work=True)
    assert fd.counters()["node_fetches"] <= 1.02 * nd.counters()["node_fetches"], (fd.counters()["node_fetches"], nd.counters()["node_fetches"])


@pytest.mark.parametrize("dist", [3.0e6, 1.0e9])
def test_far_ray_origins_end_and_hit_what_the_oracle_hits(gpu, dist):
    """from ~2^19 scene sizes away the per-ray pad of the fp32 box test exceeds the whole quantisation grid,
    so the inverted range of an unused child slot no longer rejects the ray; the traversal checks the slot's ref as
    well (descending into the empty slot lost the stack or never ended).  Rays from far outside a unit scene, aimed at
    it: every traversal ends and finds the oracle's triangle."""
    data = scenes.cornell_box(ball_subdiv=2, width=16, height=16)
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    rng = np.random.default_rng(5)
    n = 4096
    lo, hi = data.bounds()
    tgt = lo + rng.random((n, 3)) * (hi - lo)
    u = rng.normal(size=(n, 3))
    o = u / np.linalg.norm(u, axis=1, keepdims=True) * dist
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, dtype=_abi.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmin"], rays["tmax"] = o, d, 1e-4, np.inf
    b = orc.trace_closest(rays)
    for s in (sc, api.Scene(data, device_bvh=True).upload(gpu)):
        g = s.trace_closest(rays)
        assert np.array_equal(g["prim"] >= 0, b["prim"] >= 0)
        hit = b["prim"] >= 0
        assert hit.mean() > 0.5
        # t = (D - n.o) / (n.d) cancels ~dist digits
        assert np.all(np.abs(g["t"][hit] - b["t"][hit]) <= 1e-9 * dist * 1e-3 + 1e-12 * b["t"][hit])
        assert (g["prim"][hit] != b["prim"][hit]).mean() < 2e-2  # at this distance neighbouring triangles tie within rounding
    # K3 with the camera that far away (a telephoto view of the box): finishes, and the frame is the oracle's
    import copy
    cam = copy.copy(data.camera)
    eye = np.asarray(cam.look_at, dtype=np.float64) + np.array([0.05, 0.03, 1.0]) / np.linalg.norm([0.05, 0.03, 1.0]) * dist
    cam = scenes.Camera(16, 16, float(np.degrees(2 * np.arctan(1.2 / dist))), tuple(eye), tuple(cam.look_at))
    img = sc.render(camera=cam, spp=4, max_depth=4, seed=3)
    ref, _ = orc.render(camera=cam, spp=4, max_depth=4, seed=3)
    assert np.isfinite(img).all() and img.mean() > 0
    assert abs(img.mean() - ref.mean()) <= 0.05 * ref.mean()  # camera rays tie between neighbouring triangles at this distance


def test_failed_upload_leaves_scene_unusable_but_sane(gpu, dev_lib, monkeypatch):
    """a failure in the middle of prt_scene_upload must not leave a half-filled device scene behind
    (prt_sample_lights would launch on null tables).  PRT_TEST_FAIL_UPLOAD=k makes the k-th table upload report
    out-of-memory; afterwards every compute call must refuse cleanly and a later upload must work."""
    data = scenes.tiny_scene()
    sc = api.Scene(data)
    for k in (0, 2, 4, 6):
        monkeypatch.setenv("PRT_TEST_FAIL_UPLOAD", str(k))
        with pytest.raises(api.PrtError) as e:
            sc.upload(0)
        assert e.value.code == _abi.PRT_E_OOM
        for call in (lambda: sc.sample_lights(np.zeros((4, 3))), lambda: sc.render(spp=1), lambda: sc.trace_closest(np.zeros(1, dtype=_abi.RAY_DTYPE))):
            with pytest.raises(api.PrtError) as e2:
                call()
            assert e2.value.code == _abi.PRT_E_NO_DEVICE
    monkeypatch.delenv("PRT_TEST_FAIL_UPLOAD")
    sc.upload(0)
    img = sc.render(spp=2, max_depth=4, seed=3)
    ref, _ = oracle.Oracle(data).render(spp=2, max_depth=4, seed=3)
    compare_images(img, ref)
    # the same for a device-built tree (its staging copies are freed on every path)
    sd = api.Scene(data, device_bvh=True)
    monkeypatch.setenv("PRT_TEST_FAIL_UPLOAD", "1")
    with pytest.raises(api.PrtError):
        sd.upload(0)
    monkeypatch.delenv("PRT_TEST_FAIL_UPLOAD")
    sd.upload(0)
    compare_images(sd.render(spp=2, max_depth=4, seed=3), ref)


def test_negative_max_depth_renders_black(gpu):
    """Camera.cpp:121: RayColor returns 0 when depth < 0, before tracing anything — maxDepth < 0 is a black frame
    (and not the camera-ray emission / background the kernel would otherwise add)."""
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(0)
    img = sc.render(spp=3, max_depth=-1, seed=1, background=(0.3, 0.2, 0.1))
    ref, _ = oracle.Oracle(data).render(spp=3, max_depth=-1, seed=1, background=(0.3, 0.2, 0.1))
    assert not img.any() and not ref.any()
    assert sc.counters()["rays_closest"] == 0
    # depth 0 still traces the camera ray
    img0 = sc.render(spp=3, max_depth=0, seed=1, background=(0.3, 0.2, 0.1))
    ref0, _ = oracle.Oracle(data).render(spp=3, max_depth=0, seed=1, background=(0.3, 0.2, 0.1))
    compare_images(img0, ref0)
    assert img0.any()


def test_three_calls_in_flight_on_three_streams(gpu):
    """the asynchronous entry points alternate two per-call slots; a third call in flight (three streams,
    or a trace call between two pipelined renders) must wait for the call that last used its slot instead of
    resetting that call's work counter under it.  Three frames with different seeds on three streams, plus a ray
    batch in between, must equal the same frames rendered one at a time."""
    import torch
    data = scenes.cornell_box(ball_subdiv=2, width=256, height=256)
    sc = api.Scene(data).upload(0)
    cam = data.camera
    seeds = (11, 12, 13)
    want = []
    for s in seeds:
        fb = torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda")
        sc.render_device(fb.data_ptr(), None, spp=24, max_depth=6, seed=s)
        torch.cuda.synchronize()
        want.append(fb.cpu().numpy())
    lo, hi = data.bounds()
    rays = scenes.random_rays(1 << 16, lo, hi, seed=5)
    d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
    d_h = torch.zeros((rays.shape[0], 4), dtype=torch.float64, device="cuda")
    sc.trace_closest_device(d_r.data_ptr(), rays.shape[0], d_h.data_ptr())
    torch.cuda.synchronize()
    hits_want = d_h.cpu().numpy().copy()
    for rep in range(3):
        streams = [torch.cuda.Stream() for _ in seeds]
        fbs = [torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda") for _ in seeds]
        d_h.zero_()
        torch.cuda.synchronize()
        for k, (s, st, fb) in enumerate(zip(seeds, streams, fbs)):
            with torch.cuda.stream(st):
                sc.render_device(fb.data_ptr(), None, spp=24, max_depth=6, seed=s, stream=st.cuda_stream)
                if k == 0:
                    sc.trace_closest_device(d_r.data_ptr(), rays.shape[0], d_h.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize()
        for fb, w in zip(fbs, want):
            assert np.array_equal(fb.cpu().numpy(), w)
        assert np.array_equal(d_h.cpu().numpy(), hits_want)


def test_sorted_batch_returns_the_same_hits_in_the_same_places(gpu):
    """K4 (prt_trace_closest_sorted_device): the batch is traced in a locality order — keys, radix sort, K1 through the
    permutation — and hits[i] must still answer rays[i], bit for bit what the unsorted call returns: on a cache-resident
    scene, on a triangle soup, in both precisions, for batches of 0, 1 and an odd number of rays, with origins outside the
    scene's box and a NaN origin thrown in (it has to come back as a miss, not hang or move other rays' hits)."""
    import torch
    for data, n in ((scenes.cornell_box(ball_subdiv=3, width=64, height=64), 200_003), (scenes.triangle_soup(n_tris=300_000, with_light=False), 150_001)):
        sc = api.Scene(data).upload(0)
        lo, hi = data.bounds()
        rays = scenes.random_rays(n, lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), seed=9)
        rays["o"][7] = np.nan
        d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
        for prec in (0, 1):
            for m in (n, 1, 0):
                a = torch.full((max(m, 1), 4), -7.0, dtype=torch.float64, device="cuda")
                b = torch.full((max(m, 1), 4), -7.0, dtype=torch.float64, device="cuda")
                sc.trace_closest_device(d_r.data_ptr(), m, a.data_ptr(), precision=prec)
                sc.trace_closest_device(d_r.data_ptr(), m, b.data_ptr(), precision=prec, sort=True)
                torch.cuda.synchronize()
                assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
                if m == n:
                    c = sc.counters()
                    assert c["rays_closest"] == n and c["kernel_ms"] > 0
                    h = a.cpu().numpy().view(_abi.HIT_DTYPE).reshape(-1)
                    assert h["prim"][7] == -1 and (h["prim"] >= 0).mean() > 0.2
        del sc


def test_scenes_give_their_device_memory_back(gpu):
    """Create / upload / use / destroy, many times over, with every kind of call that allocates on the way (both builders,
    fp32 tables, the render partial sums, K4's sort scratch, a vertex update): the device's free memory must return to
    where it was — a renderer that serves frames for days cannot leak per scene."""
    import torch
    torch.cuda.synchronize()
    data = scenes.cornell_box(ball_subdiv=3, width=96, height=96)
    lo, hi = data.bounds()
    rays = scenes.random_rays(50_000, lo, hi, seed=2)
    d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
    d_h = torch.zeros((rays.shape[0], 4), dtype=torch.float64, device="cuda")

    def cycle(dev):
        sc = api.Scene(data, device_bvh=dev).upload(0)
        sc.render(spp=2, max_depth=3)
        sc.render(spp=2, max_depth=3, precision=1)
        sc.trace_closest_device(d_r.data_ptr(), rays.shape[0], d_h.data_ptr(), sort=True)
        sc.trace_closest_device(d_r.data_ptr(), rays.shape[0], d_h.data_ptr(), precision=1)
        torch.cuda.synchronize()
        sc.update_vertices(data.vertices * 1.01)
        sc.render(spp=1, max_depth=2)
        sc.close()

    for dev in (False, True):  # the first cycles may grow pools inside the runtime: measured after a warm-up
        cycle(dev)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for k in range(12):
        cycle(bool(k & 1))
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) / 2**20:.1f} MiB of device memory did not come back after 12 scene lifetimes"


def test_counters_report_the_tree_that_is_resident(gpu):
    """prt_get_counters' static fields follow the tree in use, host- or device-built (r1: bvh_nodes was 0 for device builds)."""
    data = scenes.cornell_box(ball_subdiv=2, width=64, height=64)
    for dev in (False, True):
        sc = api.Scene(data, device_bvh=dev).upload(0)
        sc.render(spp=1, max_depth=2)
        c, info = sc.counters(), sc.bvh_info()
        assert c["bvh_nodes"] == info["n_nodes"] > 0 and c["bvh_depth"] == info["depth"] > 0
        assert info["built_on_device"] == int(dev) and info["node_bytes"] in (32, 64) and info["width"] in (2, 4)
        lo, hi = data.bounds()
        sc.trace_closest(scenes.random_rays(5000, lo, hi, seed=3), count_work=True)
        c = sc.counters()
        assert 0 < c["tri_full"] <= c["tri_tests"]


def test_padded_and_packed_triangle_records_agree(gpu, dev_lib, monkeypatch):
    """Intersection records are packed (96 bytes apart) for scenes the caches hold and padded to one per 128-byte line
    for scenes that stream from HBM (> 256 MB of records); each layout has its own kernel instantiations.  Forcing
    the padded layout on a small scene must give bit-identical hits and frames, for both builders."""
    data = scenes.bathroom(96, 54, detail=0.15)
    lo, hi = data.bounds()
    rays = scenes.random_rays(60000, lo, hi, seed=9)
    res = {}
    for stride in ("96", "128"):
        monkeypatch.setenv("PRT_TUNE_TRI_STRIDE", stride)
        for dev in (False, True):
            sc = api.Scene(data, device_bvh=dev).upload(0)
            assert sc.bvh_info()["tri_stride"] == int(stride)
            res[(stride, dev)] = (sc.trace_closest(rays), sc.render(spp=3, max_depth=5, seed=2))
    for dev in (False, True):
        a, b = res[("96", dev)], res[("128", dev)]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    compare_hits(res[("128", False)][0], oracle.Oracle(data).trace_closest(rays))


def _random_scene(seed):
    """A random soup inside a lit box: 60-400 random triangles of random sizes spread over 3-9 meshes with materials drawn
    from all seven kinds (random parameters, some textured), one or two emissive meshes, a random camera."""
    rng = np.random.default_rng(seed)
    b = scenes._Builder(f"fuzz{seed}")
    M = scenes.Material
    ntex = int(rng.integers(0, 3))
    for _ in range(ntex):
        c = int(rng.choice([1, 3, 4]))
        shape = (int(rng.integers(2, 9)), int(rng.integers(2, 9))) + ((c,) if c > 1 else ())
        b.textures.append(rng.integers(0, 256, size=shape, dtype=np.uint8))
    def rand_mat(k):
        kind = int(rng.choice([0, 0, 1, 1, 2, 3, 5, 6]))
        tex = int(rng.integers(0, ntex)) if ntex and kind in (0, 1) and rng.random() < 0.5 else -1
        return M(f"fuzz{k}", kind, kd=tuple(rng.uniform(0.05, 0.9, 3)), ks=tuple(rng.uniform(0.05, 0.6, 3)),
                 ns=float(rng.choice([0.5, 5.0, 12.0, 60.0, 900.0])), eta=tuple(rng.uniform(0.1, 2.5, 3)), k=tuple(rng.uniform(0.0, 4.0, 3)),
                 alpha_x=float(rng.uniform(0.05, 0.8)), alpha_y=float(rng.uniform(0.05, 0.8)), texture=tex)
    box = b.material(M("DiffuseWhite", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    for name, q in (("floor", ((-2, -2, 2), (2, -2, 2), (2, -2, -2), (-2, -2, -2))), ("back", ((-2, -2, -2), (2, -2, -2), (2, 2, -2), (-2, 2, -2))),
                    ("left", ((-2, -2, 2), (-2, -2, -2), (-2, 2, -2), (-2, 2, 2))), ("right", ((2, -2, -2), (2, -2, 2), (2, 2, 2), (2, 2, -2)))):
        b.mesh(name, box, *scenes.quad(*q))
    for k in range(int(rng.integers(3, 10))):
        n = int(rng.integers(10, 60))
        c = rng.uniform(-1.5, 1.5, size=(n, 1, 3))
        size = rng.choice([0.05, 0.2, 0.6, 1.5], size=(n, 1, 1))
        v = c + size * rng.uniform(-1, 1, size=(n, 3, 3))
        uv = rng.uniform(-0.3, 1.3, size=(n, 3, 2))
        nrm = rng.normal(size=(n, 3, 3))
        b.mesh(f"soup{k}", b.material(rand_mat(k)), v, uv, nrm)
    for k in range(int(rng.integers(1, 3))):
        lm = b.material(M("Light" if k == 0 else f"light{k}", _abi.MAT_DIFFUSE_LIGHT, emission=tuple(rng.uniform(2, 20, 3))))
        y = 1.9 - 0.1 * k
        x0, z0 = rng.uniform(-1.2, 0.4, 2)
        # wound so that the light faces down, into the box
        b.mesh(f"lamp{k}", lm, *scenes.quad((x0, y, z0), (x0 + 0.8, y, z0), (x0 + 0.8, y, z0 + 0.8), (x0, y, z0 + 0.8)))
    eye = tuple(rng.uniform(-0.3, 0.3, 2)) + (float(rng.uniform(4.5, 6.0)),)
    return b.build(scenes.Camera(int(rng.integers(20, 41)), int(rng.integers(16, 33)), float(rng.uniform(35, 60)), eye, tuple(rng.uniform(-0.2, 0.2, 3))))


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_scenes_against_the_oracle(gpu, seed):
    """Property test: on random soups with random materials of every kind the HIP path and the oracle agree on closest
    hits (both BVH builders), on the light picks and on the frame — the arithmetic paths a hand-made scene does not reach
    (CookTorrance samples that leave the surface, Phong samples below the horizon, grey / RGBA textures, uv outside [0,1],
    back faces, grazing hits, overlapping triangles) are reached here by chance."""
    data = _random_scene(seed)
    orc = oracle.Oracle(data)
    lo, hi = data.bounds()
    rays = scenes.random_rays(30000, lo - 0.3, hi + 0.3, seed=seed + 100)
    want = orc.trace_closest(rays)
    for dev in (False, True):
        sc = api.Scene(data, device_bvh=dev).upload(gpu)
        compare_hits(sc.trace_closest(rays), want)
    org = np.random.default_rng(seed).uniform(-1.5, 1.5, size=(3000, 3))
    g, c = sc.sample_lights(org, seed=seed), orc.sample_lights(org, seed=seed)
    assert np.array_equal(g["prim"], c["prim"]) and np.array_equal(g["front"], c["front"])
    assert np.allclose(g["position"], c["position"], rtol=1e-13, atol=1e-13) and np.allclose(g["pdf"], c["pdf"], rtol=1e-14)
    spp, depth = 5, 7
    cpu, ccnt = orc.render(spp=spp, max_depth=depth, seed=seed + 1, background=(0.1, 0.2, 0.3))
    assert np.isfinite(cpu).all()
    img = sc.render(spp=spp, max_depth=depth, seed=seed + 1, background=(0.1, 0.2, 0.3))
    # every pixel (until round 3 this allowed 0.5 % "flipped" pixels; they were the light-pick bug — tools/fuzz_campaign.py:
    # 3,000 such scenes at spp 64, 2,157,542 pixels, none beyond 1e-9)
    compare_images(img, cpu)
    assert_ray_counts(sc.counters(), ccnt)


@pytest.mark.parametrize("scene_fn,depth", [(scenes.tiny_scene, 8), (scenes.mixed_materials, 6)])
def test_render_samples_hook_matches_the_oracle_per_sample(gpu, scene_fn, depth):
    """prt_render_samples: RayColor of single samples through K3 itself, with the path's signature (triangles hit, NEE /
    visibility / roulette / Scatter decisions per vertex).  Per (pixel, sample): the same radiance as the oracle to 1e-9 and
    the same signature; the production instantiation and the counting one give the same numbers (to rounding: since round 4 the
    counting kernels are the PRT_FEAT_EXTRA compilation, which may contract its multiply-adds differently); a frame is the mean
    of its samples."""
    data = scene_fn()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    rng = np.random.default_rng(3)
    px = np.stack([rng.integers(0, cam.width, 300), rng.integers(0, cam.height, 300)], axis=1)
    spp = 70  # more than one launch of PRT_MAX_CHUNKS samples
    g, gt = sc.render_samples(px, spp=spp, max_depth=depth, seed=4, trace=True)
    gp = sc.render_samples(px, spp=spp, max_depth=depth, seed=4)
    assert (np.abs(g - gp) <= 1e-12 * np.maximum(1.0, np.abs(gp))).all()
    o, ot = orc.render_samples(px, spp=spp, max_depth=depth, seed=4, trace=True)
    rel = np.abs(g - o) / np.maximum(1.0, np.abs(o))
    same = (gt == ot).all(-1)
    # every sample (3,456,000 samples of 3,000 random scenes: no other signature, none beyond 1e-9 — tools/fuzz_campaign.py;
    # the one event known to differ, a random draw of exactly 0, has its own test below)
    assert same.all(), int((~same).sum())
    assert (rel.max(-1) <= 1e-9).all()
    assert (gt[..., 0] >= 1).all() and (gt[..., 0] <= depth + 1).all() and gt[..., 0].max() > 3
    # sub-ranges address the same streams
    g2 = sc.render_samples(px[:5], spp=spp, max_depth=depth, seed=4, sample_begin=17, sample_count=9)
    assert np.array_equal(g2, gp[:5, 17:26])  # (gp: the production kernel, like g2; g came from the counting compilation)
    # a frame's pixel is the mean of its samples (summed in another order: rounding only)
    img = sc.render(spp=spp, max_depth=depth, seed=4)
    want = g.mean(axis=1)
    got = img[px[:, 1], px[:, 0]]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-13)


def _np_mix64(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _np_second_draw(seed, n):
    """The second 31-bit number of the streams keyed (seed, i, 0), i < n — numpy restatement of the keyed RNG (checked
    against oracle.rng_stream below), used to FIND streams with a given property among millions."""
    with np.errstate(over="ignore"):
        key = _np_mix64(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15))
        i = np.arange(n, dtype=np.uint64)
        s = _np_mix64(key ^ ((i + np.uint64(1)) << np.uint64(32)) ^ np.uint64(1))
        s0, s1 = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)
        s1 = s1 ^ s0
        s0 = ((s0 << np.uint32(26)) | (s0 >> np.uint32(6))) ^ s1 ^ (s1 << np.uint32(9))
        return (s0 * np.uint32(0x9E3779BB)) >> np.uint32(1)


def test_light_pick_wraps_around_like_traversesample_when_float_p_reaches_the_area(gpu):
    """What the 4-9 'flipped' pixels of the spp-500 headline rows were (rounds 1-2 took them for knife-edge branches): with ONE
    emissive mesh the top-level lights node is a span-1 BVHNode (left == right, BVH.cpp:21-23); for xi > 1 - 2^-24 the float
    p = sqrt(xi) * area rounds up to the whole area, `p < left->GetArea()` fails, TraverseSample descends the same child
    with p - area = 0 and picks the FIRST triangle of the CDF (BVH.cpp:93-98) — the flattened tree used to skip the span-1
    node and pick the last one.  One such xi turns up per ~1.7e7 light samples; here they are searched for."""
    assert int(_np_second_draw(7, 16)[5]) == int(round(oracle.rng_stream(7, 5, 0, 2)[1] * 2 ** 31))
    n = 1 << 16
    hits = []
    for seed in range(1, 4000):
        d = _np_second_draw(seed, n)
        idx = np.nonzero(d >= (1 << 31) - 100)[0]          # sqrt(xi) * A rounds to A for xi >= 1 - 2^-24 (128 values)
        if idx.size:
            hits.append((seed, idx))
        if len(hits) >= 4:
            break
    assert len(hits) >= 3
    for fn in (scenes.tiny_scene, lambda: scenes.cornell_box(ball_subdiv=2, width=16, height=16)):
        data = fn()
        sc = api.Scene(data).upload(gpu)
        orc = oracle.Oracle(data)
        order = orc.light_order()
        lo, hi = data.bounds()
        origins = lo + np.random.default_rng(1).random((n, 3)) * (hi - lo)
        for seed, idx in hits:
            g, c = sc.sample_lights(origins, seed=seed), orc.sample_lights(origins, seed=seed)
            assert np.array_equal(g["prim"], c["prim"]) and np.array_equal(g["pdf"], c["pdf"])
            assert (c["prim"][idx] == order[0]).all()       # the wrap-around: first triangle of the CDF, not the last
            assert np.allclose(g["position"], c["position"], rtol=0, atol=1e-14)


def test_config5_frame_in_eight_tile_shares(gpu):
    """BASELINE config 5's frame (bathroom2 1280x720, depth 50) cut the way eight ranks cut it — 16x16 tiles dealt
    diagonally — at 2 spp: the eight shares are disjoint, their sum is the full frame bit for bit, and no share traces
    more than a few percent more rays than another (that balance is what bounds 8-GPU scaling)."""
    data = scenes.bathroom()
    sc = api.Scene(data).upload(gpu)
    full = sc.render(spp=2, max_depth=50, seed=1)
    acc = np.zeros_like(full)
    covered = np.zeros(full.shape[:2], dtype=np.int32)
    rays = []
    for r in range(8):
        part = sc.render(spp=2, max_depth=50, seed=1, rank=r, nranks=8, tile_size=16)
        c = sc.counters()
        rays.append(c["rays_closest"] + c["rays_shadow"])
        covered += (part != 0).any(-1)
        acc += part
    assert np.array_equal(acc, full)
    assert covered.max() == 1
    rays = np.array(rays, dtype=np.float64)
    assert rays.max() / rays.min() <= 1.03, rays / rays.mean()


def test_headline_rows_equal_the_oracle_on_every_pixel(gpu):
    """The rows bench.py checks on the headline configuration (cornell-box 1024x1024 spp 500 depth 20): every pixel within
    1e-9 of the oracle.  Rounds 1-2 tolerated 4-9 pixels here as 'knife-edge branch flips'; per-sample signatures
    (prt_render_samples) showed identical paths with ONE different direct-light term each: the light pick's wrap-around
    (test_light_pick_wraps_around_...), a parity bug, not a knife edge.  With it fixed nothing is left to tolerate."""
    data = scenes.cornell_box()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    y0, y1 = 456, 568
    ref, _ = orc.render(spp=500, max_depth=20, seed=1, rows=(y0, y1), nthreads=16)
    img = sc.render(spp=500, max_depth=20, seed=1)
    rel = np.abs(img[y0:y1] - ref[y0:y1]) / np.maximum(1.0, np.abs(ref[y0:y1]))
    assert (rel <= 1e-9).all(), (int((rel > 1e-9).any(-1).sum()), float(rel.max()))
    assert rel.max() <= 1e-12   # observed 9e-15: summation order and last-bit arithmetic only


def test_the_one_pixel_of_the_headline_frame_that_differs_is_the_zero_draw(gpu):
    """Whole-frame parity of the headline configuration (tools/full_frame_parity.py, profiles/r03_full_frame_parity.json): ONE
    pixel of 1,048,576 is beyond 1e-9 — (296, 161), through sample 465 alone.  It is a true knife edge with a known trigger:
    the sixth number of that sample's stream is exactly 0 (probability 2^-31 per draw), it is the first draw of the cosine
    sample at the camera vertex, so the concentric map lands ON the unit circle (r = -1) and z = sqrt(max(0, 1 - x^2 - y^2))
    is 0 or ~1e-8 depending on the last bit of cos^2 + sin^2 — the reference's `while (wi.z <= 0)` (Material.h:111-116)
    redraws on one side of that bit and not on the other (glibc's sin / cos there, the fdlibm kernels here).  Every other
    sample of the pixel agrees to 1e-9, and the signatures agree up to that vertex."""
    data = scenes.cornell_box()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    px = [[296, 161]]
    g, gt = sc.render_samples(px, spp=500, max_depth=20, seed=1, trace=True)
    o, ot = orc.render_samples(px, spp=500, max_depth=20, seed=1, trace=True)
    rel = (np.abs(g[0] - o[0]) / np.maximum(1.0, np.abs(o[0]))).max(-1)
    differing = np.nonzero(rel > 1e-9)[0].tolist()
    assert differing in ([465], []), differing     # ([]: should both sides ever round that bit the same way)
    stream = oracle.rng_stream(1, 161 * cam.width + 296, 465, 8)
    assert stream[5] == 0.0                        # draws 0-3 light pick, 4 roulette, 5-6 the cosine sample: u.y = 0 -> r = -1
    assert gt[0, 465, 1] == ot[0, 465, 1] and gt[0, 465, 2] == ot[0, 465, 2]   # same camera vertex, same decisions there


@pytest.mark.parametrize("name,factory,depth", [("cornell-box", "cornell_box", 20), ("veach-mis", "veach_mis", 100), ("bathroom2", "bathroom", 50)])
def test_whole_frame_equals_the_oracle_on_every_pixel(gpu, name, factory, depth):
    """whole-frame parity under the driver's eyes.  The three BASELINE scenes at their full resolution and
    their configuration's depth, spp 8, EVERY pixel against the oracle's frame (all host threads as row workers,
    Camera.cpp:46-71's split): none beyond 1e-9 — and nothing near it (observed maxima ~1e-13, rounding order only)."""
    data = getattr(scenes, factory)()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    ref, ocnt = orc.render(spp=8, max_depth=depth, seed=1, nthreads=min(64, len(os.sched_getaffinity(0))))
    img = sc.render(spp=8, max_depth=depth, seed=1)
    assert img.shape == ref.shape == (cam.height, cam.width, 3)
    rel = np.abs(img - ref) / np.maximum(1.0, np.abs(ref))
    bad = (rel > 1e-9).any(-1)
    assert bad.sum() == 0, (name, int(bad.sum()), np.argwhere(bad)[:8].tolist(), float(rel.max()))
    assert rel.max() <= 1e-10, float(rel.max())
    cnt = sc.counters()
    assert cnt["samples"] == ocnt["samples"] == cam.width * cam.height * 8
    sc.close()


def test_texture_footprints_have_a_ceiling(gpu):
    """VERDICT r3 #6 (ImageTexture::Value, Source/Texture.cpp:22-71): textures are stored as bilinear footprints (128 bytes per
    texel, one line per lookup) only while ALL of a scene's footprints stay within 256 MiB; a scene beyond that keeps plain
    texel arrays (24 bytes per texel) — one layout per scene, so the kernel's choice is a scalar branch.  A 4096^2 map next to
    a 512^2 one: the scene uploads in < 0.5 GB of texels instead of 2.2 GB, and the frame equals the oracle's."""
    import copy
    data = copy.copy(scenes.bathroom(96, 54, detail=0.15))
    big = np.tile(data.textures[0], (8, 8, 1))                   # 4096 x 4096 x 3
    assert big.shape == (4096, 4096, 3)
    data.textures = [big, data.textures[1]]
    sc = api.Scene(data).upload(gpu)
    info = sc.bvh_info()
    assert info["texture_layouts"] == 2 and info["texture_footprint_bytes"] == 0          # plain texel arrays
    assert info["texture_bytes"] == (512 * 512 + 4096 * 4096) * 24 < 0.5e9                # (as footprints: 2.2 GB)
    img = sc.render(spp=4, max_depth=6, seed=5)
    ref, _ = oracle.Oracle(data).render(spp=4, max_depth=6, seed=5, nthreads=8)
    compare_images(img, ref)
    # the fp32 fast mode derives its tables from the same array (either layout)
    img32 = sc.render(spp=4, max_depth=6, seed=5, precision=1)
    assert np.isfinite(img32).all() and abs(img32.mean() - ref.mean()) <= 2e-3 * ref.mean()
    sc.close()
    # the stand-in scenes are far below the ceiling: footprints, as measured in DESIGN.md
    small = api.Scene(scenes.bathroom(96, 54, detail=0.15)).upload(gpu)
    assert small.bvh_info()["texture_layouts"] == 1 and small.bvh_info()["texture_bytes"] == 2 * 512 * 512 * 128
    assert small.bvh_info()["texture_footprint_bytes"] == 2 * 512 * 512 * 128


def test_texture_layouts_give_the_same_frame(gpu, dev_lib, monkeypatch):
    """Same doubles, same blend: with the footprint budget forced to 0 (dev-hooks library) every texture stays a plain texel
    array; the texture lookups are the footprint build's bit for bit (same kernel), the frame to rounding (the scene then runs
    the PRT_FEAT_EXTRA compilation of K3: another kernel, other FMA contractions)."""
    data = scenes.bathroom(96, 54, detail=0.15)
    a = api.Scene(data).upload(gpu)
    assert a.bvh_info()["texture_layouts"] == 1
    monkeypatch.setenv("PRT_TUNE_TEX_BUDGET", "0")
    b = api.Scene(data).upload(gpu)
    assert b.bvh_info()["texture_layouts"] == 2 and b.bvh_info()["texture_footprint_bytes"] == 0
    kw = dict(spp=4, max_depth=6, seed=5)
    ia, ib = a.render(**kw), b.render(**kw)
    assert (np.abs(ia - ib) <= 1e-12 * np.maximum(1.0, np.abs(ib))).all()
    uv = np.random.default_rng(3).uniform(-0.2, 1.2, size=(4096, 2))
    assert np.array_equal(a.texture_value(0, uv), b.texture_value(0, uv))


def test_many_materials_on_a_deep_tree_keep_their_occupancy(gpu):
    """ADVICE r3 (prt_api.cpp, LDS budget): the fp64 render kernels keep static 40-entry stacks, so their table budget is what
    THOSE leave at the permutation's occupancy — a deep host-built tree with ~35 materials used to be moved to the 32-entry
    tree and given tables sized for stacks the kernel does not have, which cost a resident block.  Now: the full tree, and
    tables only when the occupancy query says they cost nothing."""
    import copy
    base = scenes.bathroom(96, 54, detail=1.0)        # 126k triangles: the deep tree of BASELINE config 4
    for extra in (0, 25, 60):
        data = copy.copy(base)
        data.materials = list(base.materials) + [base.materials[3]] * extra
        sc = api.Scene(data).upload(gpu)
        info = sc.bvh_info()
        assert info["stack_need"] > 32                                            # a tree the 32-entry collapse would change
        assert info["render_blocks_per_cu"] == info["render_blocks_wanted"] == 3, info   # textured permutation: three blocks per CU
        if extra == 0:
            assert info["lds_materials"] == len(data.materials)                   # ten materials fit beside the stacks
            ref_img = sc.render(spp=2, max_depth=6, seed=9)
        else:
            # more materials than the ~5 KB beside three blocks' stacks hold: no tables, still three blocks; same frame
            assert info["lds_materials"] in (0, len(data.materials))
            # (the kernels with and without LDS tables are separate compilations: FMA contraction may differ, the tolerance applies)
            compare_images(sc.render(spp=2, max_depth=6, seed=9), ref_img)
        sc.close()
