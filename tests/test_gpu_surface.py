"""GPU tests of the surface queries (prt_trace_surface*, Scene.trace_surface*, the batch Hittable::Hit).

Two statements carry everything else.  The head of a record — its first 32 bytes — is the PrtHit the closest-hit call
writes for the same ray record and precision, bit for bit: no tolerance, no excluded rays.  The body is a pure function of
that head, the ray and the scene, restated in numpy by tests/surface_model.py and compared within the project's hit
tolerance (1e-12) for the geometry and its image tolerance (1e-9) for texture lookups; what reads no texture is exact.
Batches have 3 * 1024 + 37 rays: neither a multiple of the 64-lane wave nor of the 1024-ray pool chunk."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, build, scenes
from tests import surface_model as M
from tests.test_gpu_occlusion import _closest, _dev, _finite_tmax

pytestmark = pytest.mark.gpu

BUILDERS = (False, True)   # Scene(device_bvh=...)
N = 3 * 1024 + 37
SCENES = {"mixed": lambda: scenes.mixed_materials(48, 48), "tiny": scenes.tiny_scene}
PRECISIONS = (_abi.PRECISION_F64, _abi.PRECISION_F32)
F32_TEXTURED_ALBEDO_BOUND = 2e-5  # 4 x the largest gap measured on `mixed` (3.89e-6), rounded up to one digit: test 8's docstring


def _surface(sc, rays, precision=0, sort=False, count_work=False, d_r=None, extra=0):
    """The n records (and, with `extra`, the bytes behind them of a buffer prefilled with 0xAA)."""
    import torch
    n = rays.shape[0]
    d_r = _dev(rays) if d_r is None else d_r
    d_o = torch.full((n * 192 + max(extra, 32),), 0xAA, dtype=torch.uint8, device="cuda")
    assert d_o.data_ptr() % 32 == 0
    sc.trace_surface_device(d_r.data_ptr(), n, d_o.data_ptr(), count_work=count_work, precision=precision, sort=sort)
    torch.cuda.synchronize()
    raw = d_o.cpu().numpy()
    out = raw[:n * 192].view(_abi.SURFACE_DTYPE)
    return (out, raw[n * 192:]) if extra else out


def _head_bytes(rec):
    return rec.view(np.uint8).reshape(-1, 192)[:, :32]


def _hit_bytes(hits):
    return hits.view(np.uint8).reshape(-1, 32)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def _texture_lookup(name):
    """oracle.Oracle.texture_value of the scene's textures (the oracle lives as long as the test session)."""
    return oracle.Oracle(_scene(name)).texture_value


@functools.lru_cache(maxsize=None)
def _batches(name):
    """(rays with tmax = inf, the same rays with a finite tmax each): half random rays in the scene's bounds, half camera
    rays.  The finite lengths are drawn around the oracle's hit distances."""
    data = _scene(name)
    lo, hi = data.bounds()
    rays = np.concatenate([scenes.random_rays(N // 2, lo, hi, seed=91), scenes.camera_rays(data.camera, N - N // 2, seed=92)])
    assert rays.shape[0] == N and N % 64 and N % 1024
    orc = oracle.Oracle(data)
    t = orc.trace_closest(rays)["t"]
    orc.close()
    finite = _finite_tmax(rays, t, seed=93)
    for a in (rays, finite):
        a.setflags(write=False)
    return rays, finite


def check_heads(sc, batches, precisions=PRECISIONS):
    """Test 1 on an uploaded scene: every record's first 32 bytes against trace_closest_device on the same device buffer."""
    seen_hit = seen_miss = False
    for batch in batches:
        d_r = _dev(batch)
        for prec in precisions:
            for sort in (False, True):
                want = _closest(sc, batch, precision=prec, sort=sort, d_r=d_r)
                got = _surface(sc, batch, precision=prec, sort=sort, d_r=d_r)
                diff = (_head_bytes(got) != _hit_bytes(want)).any(1)
                print(f"prec={prec} sort={sort} finite={bool(np.isfinite(batch['tmax']).all())}: {batch.shape[0]} rays, "
                      f"{int((want['prim'] >= 0).sum())} hits, heads that differ {int(diff.sum())}")
                assert not diff.any()
                seen_hit |= bool((want["prim"] >= 0).any())
                seen_miss |= bool((want["prim"] < 0).any())
    assert seen_hit and seen_miss


def body_gaps(got, want, rays, data):
    """Largest gap per group of fields between device records and the model's, after the exact parts were asserted."""
    hit = got["prim"] >= 0
    assert np.array_equal(got["material"], want["material"]) and np.array_equal(got["material_type"], want["material_type"])
    assert (got["reserved"] == 0).all()
    miss = M.miss_record().tobytes()
    assert all(r.tobytes() == miss for r in got[~hit])
    g, w, r = got[hit], want[hit], rays[hit]
    textured = np.array([data.materials[m].texture >= 0 and data.materials[m].type in (0, 1, 5) for m in g["material"]], bool)
    pos_bound = 4 * 2.0 ** -53 * (np.abs(r["o"]) + np.abs(g["t"][:, None] * r["d"]))
    gaps = {
        "position/bound": float((np.abs(g["position"] - w["position"]) / pos_bound).max()),
        "normal": float(np.abs(g["normal"] - w["normal"]).max()),
        "tangent": float(np.abs(g["tangent"] - w["tangent"]).max()),
        "uv": float(np.abs(g["uv"] - w["uv"]).max()),
        "albedo(textured)": float(np.abs(g["albedo"][textured] - w["albedo"][textured]).max()) if textured.any() else 0.0,
        "albedo(plain)": float(np.abs(g["albedo"][~textured] - w["albedo"][~textured]).max()),
        "emission": float(np.abs(g["emission"] - w["emission"]).max()),
    }
    return gaps, int(hit.sum()), int(textured.sum())


def check_bodies(sc, data, batches, texture_value, vertices=None):
    """Test 2 on an uploaded scene (fp64): the body against the model fed with the record's own head."""
    for batch in batches:
        for sort in (False, True):
            got = _surface(sc, batch, sort=sort)
            want = M.records(data, batch, got, texture_value, vertices=vertices)
            gaps, n_hit, n_tex = body_gaps(got, want, batch, data)
            print(f"sort={sort}: {n_hit} hits ({n_tex} textured), gaps {gaps}")
            assert n_hit > batch.shape[0] // 4
            assert gaps["position/bound"] <= 1.0          # two roundings, with or without contraction
            assert max(gaps["normal"], gaps["tangent"], gaps["uv"]) <= 1e-12
            assert gaps["albedo(textured)"] <= 1e-9
            assert gaps["albedo(plain)"] == 0.0 and gaps["emission"] == 0.0
    return got


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_head_equals_closest_hit_bit_for_bit(gpu, name, device_bvh):
    sc = api.Scene(_scene(name), device_bvh=device_bvh).upload(gpu)
    check_heads(sc, _batches(name))
    sc.close()


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_body_equals_the_model(gpu, name, device_bvh):
    data = _scene(name)
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    got = check_bodies(sc, data, _batches(name), _texture_lookup(name))
    if name == "mixed":  # every material kind is met, the textured Lambertian and the textured Phong included
        kinds = set(got["material_type"][got["prim"] >= 0].tolist())
        assert kinds == {0, 1, 2, 3, 4, 5, 6}, kinds
        met = set(got["material"][got["prim"] >= 0].tolist())
        assert {i for i, m in enumerate(data.materials) if m.texture >= 0} <= met
    sc.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("hook", ["PRT_TUNE_TRI_STRIDE", "PRT_TUNE_TEX_BUDGET"])
def test_forced_layouts(gpu, dev_lib, monkeypatch, hook, device_bvh):
    """Records padded to one per 128-byte line (the PAD instantiations) and textures kept as plain texel arrays (the other
    path of the texture fetch): layouts that only scenes far beyond a test's size get by themselves."""
    monkeypatch.setenv(hook, "128" if hook == "PRT_TUNE_TRI_STRIDE" else "0")
    data = _scene("mixed")
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    info = sc.bvh_info()
    if hook == "PRT_TUNE_TRI_STRIDE":
        assert info["tri_stride"] == 128
    else:
        assert info["texture_layouts"] == 2
    check_heads(sc, _batches("mixed"))
    check_bodies(sc, data, _batches("mixed"), _texture_lookup("mixed"))
    sc.close()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", sorted(SCENES))
def test_features_are_the_camera_ray_special_case(gpu, name):
    data = _scene(name)
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    feat = sc.features(seed=3)
    cr = oracle.camera_rays(cam).reshape(-1, 6)
    rays = np.zeros(cr.shape[0], dtype=_abi.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmin"], rays["tmax"] = cr[:, :3], cr[:, 3:], 1e-4, np.inf
    got = _surface(sc, rays)
    assert np.array_equal(got["prim"], feat["prim"].reshape(-1))  # every pixel: these rays have no knife-edge pixel on these scenes
    hit = got["prim"] >= 0
    assert 0.5 < hit.mean()
    fa, fn, fz = feat["albedo"].reshape(-1, 3), feat["normal"].reshape(-1, 3), feat["depth"].reshape(-1)
    gap_a = np.abs(got["albedo"][hit].astype(np.float32) - fa[hit]).max()
    gap_n = np.abs(got["normal"][hit].astype(np.float32) - fn[hit]).max()
    z = (got["t"][hit] * np.sqrt((rays["d"][hit] ** 2).sum(1))).astype(np.float32)
    gap_z = (np.abs(z - fz[hit]) / fz[hit]).max()
    print(f"{name}: {int(hit.sum())} of {hit.size} pixels hit; gaps albedo {gap_a:.3g} normal {gap_n:.3g} depth (relative) {gap_z:.3g}")
    assert gap_a <= 1e-6 and gap_n <= 1e-6 and gap_z <= 1e-6
    assert (fa[~hit] == 1).all() and (fn[~hit] == 0).all() and np.isposinf(fz[~hit]).all()
    sc.close()


# ------------------------------------------------------------------------------------------------ 5
def test_bounds_and_alignment(gpu):
    import torch
    sc = api.Scene(_scene("mixed")).upload(gpu)
    rays = _batches("mixed")[0]
    for prec in PRECISIONS:
        full = _surface(sc, rays, precision=prec)
        for n in (N, 1, 0):
            for sort in (False, True):
                got, tail = _surface(sc, rays[:n], precision=prec, sort=sort, extra=4096)
                assert tail.size == 4096 and (tail == 0xAA).all(), (n, sort)
                assert got.tobytes() == full[:n].tobytes(), (n, sort)
    # a buffer that is not 32-byte aligned is refused and nothing is written
    d_r = _dev(rays)
    d_o = torch.full((N * 192 + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    for sort in (False, True):
        for off in (8, 16):
            with pytest.raises(api.PrtError) as e:
                sc.trace_surface_device(d_r.data_ptr(), N, d_o.data_ptr() + off, sort=sort)
            assert e.value.code == _abi.PRT_E_INVALID and "32-byte aligned" in str(e.value)
    torch.cuda.synchronize()
    assert bool((d_o == 0xAA).all())
    # the other argument checks, as the occlusion calls make them
    for sort in (False, True):
        for args in ((None, 4, d_o.data_ptr()), (d_r.data_ptr(), 4, None)):
            with pytest.raises(api.PrtError) as e:
                sc.trace_surface_device(*args, sort=sort)
            assert e.value.code == _abi.PRT_E_INVALID
        with pytest.raises(api.PrtError) as e:
            sc.trace_surface_device(d_r.data_ptr(), 4, d_o.data_ptr(), precision=7, sort=sort)
        assert e.value.code == _abi.PRT_E_INVALID
        sc.trace_surface_device(None, 0, None, sort=sort)
    with pytest.raises(api.PrtError) as e:
        sc.trace_surface_device(d_r.data_ptr(), 1 << 32, d_o.data_ptr(), sort=True)
    assert e.value.code == _abi.PRT_E_INVALID
    torch.cuda.synchronize()
    assert bool((d_o == 0xAA).all())
    sc.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_counters(gpu, device_bvh):
    sc = api.Scene(_scene("mixed"), device_bvh=device_bvh).upload(gpu)
    rays = _batches("mixed")[1]
    d_r = _dev(rays)
    for prec in PRECISIONS:
        for sort in (False, True):
            _surface(sc, rays, precision=prec, sort=sort, d_r=d_r)
            c = sc.counters()
            assert c["rays_closest"] == N and c["rays_shadow"] == 0 and c["samples"] == 0 and c["kernel_ms"] > 0
            _surface(sc, rays, precision=prec, sort=sort, count_work=True, d_r=d_r)
            c = sc.counters()
            assert c["rays_closest"] == N and c["rays_shadow"] == 0 and c["samples"] == 0
            _closest(sc, rays, precision=prec, sort=sort, count_work=True, d_r=d_r)
            k = sc.counters()
            assert k["node_fetches"] > 0 and k["tri_tests"] > 0
            for f in ("node_fetches", "tri_tests", "tri_full"):
                assert c[f] == k[f], (f, prec, sort)
    sc.close()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_records_follow_a_device_refit(gpu, device_bvh):
    import torch
    data = _scene("mixed")
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    batches = _batches("mixed")
    before = _surface(sc, batches[0])
    d_v = torch.from_numpy(np.ascontiguousarray(data.vertices, dtype=np.float64)).cuda()
    first = np.asarray(data.mesh_first_tri, np.int64)
    for ball, centre in (("goldBall", (-0.4, -0.7, -0.2)), ("texBall", (0.45, -0.75, 0.1))):  # both balls grow; the emitters stay
        m = data.mesh_names.index(ball)
        c = torch.tensor(centre, dtype=torch.float64, device="cuda")
        d_v[first[m]:first[m + 1]] = c + 1.3 * (d_v[first[m]:first[m + 1]] - c)
    sc.refit_device(d_v.data_ptr())
    assert sc.refit_info()["host_stale"] == 1
    moved = d_v.cpu().numpy()
    check_heads(sc, batches)
    check_bodies(sc, data, batches, _texture_lookup("mixed"), vertices=moved)
    after = _surface(sc, batches[0])
    both = (before["prim"] >= 0) & (after["prim"] >= 0)
    changed = int((before["normal"][both] != after["normal"][both]).any(1).sum())
    print(f"device_bvh={device_bvh}: {changed} of {int(both.sum())} hit rays see another normal after the refit")
    assert changed >= 1
    sc.close()


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_fp32_records_within_tier_two(gpu, device_bvh):
    """fp32 records against the fp64 records of the same rays, where both name the same triangle.  The head's equality with
    the fp32 closest-hit call is test 1's.  Textured albedo has no derived bound: the fp32 lookup rounds uv, the texel
    coordinates and twelve taps.  Largest gap to the fp64 record measured on `mixed` (both builders, both batches): 3.89e-6;
    the bound asserted is 4 x that, rounded up to one digit — the margin the guided filter's variance test uses."""
    data = _scene("mixed")
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    lo, hi = data.bounds()
    extent = float((np.asarray(hi) - np.asarray(lo)).max())
    worst_tex = 0.0
    for batch in _batches("mixed"):
        d_r = _dev(batch)
        r64 = _surface(sc, batch, d_r=d_r)
        r32 = _surface(sc, batch, precision=_abi.PRECISION_F32, d_r=d_r)
        same = (r64["prim"] == r32["prim"]) & (r64["prim"] >= 0)
        assert same.sum() > 0.9 * (r64["prim"] >= 0).sum()
        a, b = r64[same], r32[same]
        assert np.array_equal(a["material"], b["material"]) and np.array_equal(a["material_type"], b["material_type"])
        textured = np.array([data.materials[m].texture >= 0 and data.materials[m].type in (0, 1, 5) for m in a["material"]], bool)
        gaps = {f: float(np.abs(a[f] - b[f]).max()) for f in ("position", "normal", "tangent", "uv")}
        plain = float((np.abs(a["albedo"][~textured] - b["albedo"][~textured]) / np.maximum(np.abs(a["albedo"][~textured]), 1e-300)).max())
        em = a["emission"] != 0
        emis = float((np.abs(a["emission"] - b["emission"])[em] / np.abs(a["emission"][em])).max())
        assert ((b["emission"] == 0) == ~em).all()
        tex = float(np.abs(a["albedo"][textured] - b["albedo"][textured]).max())
        worst_tex = max(worst_tex, tex)
        print(f"device_bvh={device_bvh}: {int(same.sum())} rays on the same triangle ({int(textured.sum())} textured); gaps {gaps}, "
              f"plain albedo (relative) {plain:.3g}, emission (relative) {emis:.3g}, textured albedo {tex:.3g}")
        assert gaps["position"] <= 1e-5 * extent
        assert max(gaps["normal"], gaps["tangent"], gaps["uv"]) <= 1e-5
        assert plain <= 2.0 ** -23 and emis <= 2.0 ** -23
        assert textured.sum() > 50
    print(f"device_bvh={device_bvh}: largest textured-albedo gap fp32 against fp64 {worst_tex:.3g}")
    assert worst_tex <= F32_TEXTURED_ALBEDO_BOUND
    sc.close()


# ------------------------------------------------------------------------------------------------ 9
def test_host_call_equals_device_call(gpu):
    sc = api.Scene(_scene("mixed")).upload(gpu)
    for batch in _batches("mixed"):
        host = sc.trace_surface(batch)
        assert host.dtype == _abi.SURFACE_DTYPE and host.shape == (N,)
        assert host.tobytes() == _surface(sc, batch).tobytes()
        c = sc.counters()
        assert c["rays_closest"] == N and c["rays_shadow"] == 0
    assert sc.trace_surface(batch[:0]).shape == (0,)
    sc.close()


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_cpp_batch_hit_agrees_with_single_hit(gpu, tmp_path, device_bvh):
    """Hittable::Hit(rays, domain, records) against the single-ray Hittable::Hit on main.cpp's world."""
    build.build_host_example()
    exe = str(tmp_path / "surface_check")
    lib_dir = os.path.dirname(build.HOST_LIB)
    root = os.path.dirname(lib_dir)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "surface_check.cpp"), "-L", lib_dir,
                           "-Wl,-rpath," + lib_dir, "-lpooraytracer_host", "-lprt_hip", "-o", exe])
    data = scenes.cornell_box(ball_subdiv=2, width=48, height=40)
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    r = subprocess.run([exe, res, data.name, "400", "1" if device_bvh else "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    words = r.stdout.split()
    n, hits, bad = int(words[1]), int(words[3]), int(words[5])
    assert n == 400 and bad == 0 and 0.1 * n < hits < n
