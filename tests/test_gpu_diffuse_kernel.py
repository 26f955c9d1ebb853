"""The DIFFUSE form of the PLAIN render kernel K3 (-m gpu).  A PLAIN launch (tests/test_gpu_plain_kernel.py)
of the lean fp64 permutation in a scene whose material table holds nothing but untextured Lambertians and emitters, none of which
skips light sampling, launches k_render<false, FEAT | PRT_FEAT_PLAIN | PRT_FEAT_DIFFUSE, true, PAD>: Eval and Scatter are their
Lambertian case without a test of the material type, no vertex skips its light pick, prev_skip is not carried.  The dev-hooks
library's PRT_TUNE_NO_DIFFUSE=1 keeps a qualifying launch on the PLAIN kernel, PRT_TUNE_GENERIC=1 keeps every launch on the generic
one (and wins over the former); prt_last_render_form() answers PLAIN for a DIFFUSE launch, prt_last_render_subform() tells them apart.

  1. DIFFUSE equals PLAIN equals generic, bit for bit: the fp64 framebuffer and both ray counters of
     scenes.cornell_box(ball_subdiv=2, width=48, height=40) at spp 8, depth 6 — with a host-built and a device-built tree, on a tile
     share, at depth 1 (every path ends at its first bounce) and at spp 1 (every work item is a single sample).
  2. Ties.  The default camera of the stand-in sits off the box axis precisely so that NO pixel-centre ray meets two triangles at a
     bit-identical t (scenes.py, cornell_box; tests/test_gpu_parity.py renders it bit-identically from any tree), so the frame of
     case 1 has no such pixel.  The tie case therefore renders the same scene, same size, through symmetric_camera=True, whose
     diagonal pixel-centre rays run exactly through the edges between walls, floor and ceiling: the first two hits of such a ray
     (prt_trace_multi) have the same t and belong to meshes of different materials.  The test asserts that the 48 x 40 frame has
     such pixels and that they are lit in the frame all three forms agree on.
  3. Selection: a mirror ball, a wall that skips light sampling (an Empty material), a Debug wall and the CookTorrance ball each launch
     PLAIN and not DIFFUSE, with the same bits under both switches; the launches that are generic today (pixel jitter, sample_lights
     off, render_samples, count_work, ray_color, fp32) report neither form.
  4. The flag follows the table.  No call changes the materials of a scene after prt_scene_create (refit, rebuild and light updates
     move vertices only), so there is no path to replace one material of a resident scene: the flag is asserted on fresh uploads
     instead — a qualifying scene, the same scene with a mirror ball, and the qualifying scene again, alternating inside one library.
"""
import dataclasses

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, distributed, scenes

pytestmark = pytest.mark.gpu
F32 = _abi.PRECISION_F32
PLAIN, GENERIC = _abi.RENDER_FORM_PLAIN, _abi.RENDER_FORM_GENERIC
DIFFUSE, NONE = _abi.RENDER_SUBFORM_DIFFUSE, _abi.RENDER_SUBFORM_NONE
KW = dict(spp=8, max_depth=6, seed=1)
SWITCHES = ("PRT_TUNE_NO_DIFFUSE", "PRT_TUNE_GENERIC")
_DATA = {}


def _cornell(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _DATA:
        _DATA[key] = scenes.cornell_box(ball_subdiv=2, width=48, height=40, **kw)
    return _DATA[key]


def _with_material(data, name, **changes):
    """`data` with the material called `name` replaced (same slot, same meshes)."""
    mats = [dataclasses.replace(m, **changes) if m.name == name else m for m in data.materials]
    assert mats != list(data.materials)
    return dataclasses.replace(data, materials=mats)


def _forms(sc):
    return api.last_render_form(sc._L), api.last_render_subform(sc._L)


def _set(monkeypatch, on=()):
    for name in SWITCHES:
        if name in on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def _frame(sc, monkeypatch, on=(), **kw):
    """One frame, its ray counts and the (form, sub-form) of its launch, with the switches `on` set."""
    _set(monkeypatch, on)
    img = sc.render(**{**KW, **kw})
    cnt = sc.counters()
    _set(monkeypatch)
    return img, (cnt["rays_closest"], cnt["rays_shadow"]), _forms(sc)


def _assert_all_forms_agree(sc, monkeypatch, as_launched, where, **kw):
    """The frame as launched, under PRT_TUNE_NO_DIFFUSE=1, under PRT_TUNE_GENERIC=1 and under both: the forms as expected, the same
    bits, the same rays.  `as_launched`: (form, sub-form) of the plain launch."""
    a, rays_a, forms_a = _frame(sc, monkeypatch, **kw)
    assert forms_a == as_launched, (where, forms_a)
    assert a.max() > 0 and rays_a[0] > 0, where
    no_diffuse = (as_launched[0], NONE)  # the switch takes the sub-form away and nothing else
    for on, want in ((SWITCHES[:1], no_diffuse), (SWITCHES[1:], (GENERIC, NONE)), (SWITCHES, (GENERIC, NONE))):
        b, rays_b, forms_b = _frame(sc, monkeypatch, on, **kw)
        assert forms_b == want, (where, on, forms_b)
        assert np.array_equal(a, b), (where, on, int((a != b).sum()))
        assert rays_a == rays_b, (where, on)
    return a


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("device_bvh", [False, True], ids=["host-tree", "device-tree"])
def test_diffuse_frame_equals_plain_and_generic_frame(gpu, dev_lib, monkeypatch, device_bvh):
    assert dev_lib.prt_dev_hooks() == 1
    sc = api.Scene(_cornell(), device_bvh=device_bvh).upload(gpu)
    assert bool(sc.bvh_info()["built_on_device"]) == device_bvh
    _assert_all_forms_agree(sc, monkeypatch, (PLAIN, DIFFUSE), ("cornell", device_bvh))
    sc.close()


def test_diffuse_equals_plain_on_a_tile_share(gpu, dev_lib, monkeypatch):
    sc = api.Scene(_cornell()).upload(gpu)
    share = dict(rank=1, nranks=3, tile_size=16)
    img = _assert_all_forms_agree(sc, monkeypatch, (PLAIN, DIFFUSE), "share", **share)
    own = distributed.owned_mask(48, 40, share["tile_size"], share["rank"], share["nranks"])
    assert 0 < own.sum() < own.size and img[own].any() and not img[~own].any()
    sc.close()


@pytest.mark.parametrize("kw", [dict(max_depth=1), dict(spp=1)], ids=["depth1", "spp1"])
def test_diffuse_equals_plain_at_depth_1_and_at_spp_1(gpu, dev_lib, monkeypatch, kw):
    sc = api.Scene(_cornell()).upload(gpu)
    _assert_all_forms_agree(sc, monkeypatch, (PLAIN, DIFFUSE), kw, **kw)
    sc.close()


# ------------------------------------------------------------------------------------------------ 2
def _pixel_centre_rays(cam):
    """The camera rays through the pixel centres, in pixel order: scenes.camera_rays without its jitter."""
    W, H = cam.width, cam.height
    eye, look, up = (np.asarray(v, dtype=np.float64) for v in (cam.eye, cam.look_at, cam.up))
    el = eye - look
    focal = np.sqrt(el @ el)
    vh = 2.0 * np.tan(np.radians(cam.fovy) / 2.0) * focal
    vw = vh * (W / H)
    w = el / focal
    u = np.cross(up, w)
    u /= np.sqrt(u @ u)
    v = np.cross(w, u)
    du, dv = vw * u / W, vh * (-v) / H
    p00 = eye - focal * w - vw * u / 2.0 - vh * (-v) / 2.0 + 0.5 * (du + dv)
    k = np.arange(W * H)
    rays = np.zeros(W * H, dtype=_abi.RAY_DTYPE)
    rays["o"] = eye
    rays["d"] = p00 + (k % W)[:, None] * du + (k // W)[:, None] * dv - eye
    rays["tmin"] = 1e-4
    rays["tmax"] = np.inf
    return rays


def test_diffuse_equals_plain_on_a_frame_with_exact_ties(gpu, dev_lib, monkeypatch):
    data = _cornell(symmetric_camera=True)
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    two = sc.trace_multi(_pixel_centre_rays(cam), 2)
    mesh_of = np.searchsorted(data.mesh_first_tri.astype(np.int64), two["prim"], side="right") - 1
    mat_of = np.asarray(data.mesh_material)[mesh_of]
    tie = (two["prim"][:, 1] >= 0) & (two["t"][:, 0] == two["t"][:, 1]) & (mat_of[:, 0] != mat_of[:, 1])
    print(f"[diffuse] {int(tie.sum())} of {tie.size} pixel-centre rays meet two materials at a bit-identical t")
    assert tie.sum() >= 4, int(tie.sum())
    jj, ii = np.divmod(np.flatnonzero(tie), cam.width)
    assert (np.abs(ii - (cam.width - 1) / 2) == np.abs(jj - (cam.height - 1) / 2)).all()  # the image diagonals, where x = +-y
    img = _assert_all_forms_agree(sc, monkeypatch, (PLAIN, DIFFUSE), "ties")
    assert (img[jj, ii] > 0).any(-1).all()
    # ... and the off-axis camera of case 1 has none (module docstring)
    off = api.Scene(_cornell()).upload(gpu)
    two = off.trace_multi(_pixel_centre_rays(off.data.camera), 2)
    assert not ((two["prim"][:, 1] >= 0) & (two["t"][:, 0] == two["t"][:, 1])).any()
    off.close()
    sc.close()


# ------------------------------------------------------------------------------------------------ 3
NOT_DIFFUSE = {
    "mirror-ball": lambda: _with_material(_cornell(), "DiffuseBall", type=_abi.MAT_MIRROR),
    "wall-skips-light-sampling": lambda: _with_material(_cornell(), "RightWall", type=_abi.MAT_EMPTY),  # Empty: SkipLightSampling, no Scatter
    "debug-wall": lambda: _with_material(_cornell(), "LeftWall", type=_abi.MAT_DEBUG),  # emits its albedo: two more light triangles
    "cooktorrance-ball": lambda: _cornell(ball_cooktorrance_alpha=0.1),
}


@pytest.mark.parametrize("case", list(NOT_DIFFUSE))
def test_scenes_that_must_not_be_diffuse_are_plain(gpu, dev_lib, monkeypatch, case):
    sc = api.Scene(NOT_DIFFUSE[case]()).upload(gpu)
    _assert_all_forms_agree(sc, monkeypatch, (PLAIN, NONE), case)
    sc.close()


def _expect_generic(sc, monkeypatch, what, call):
    """`call()` under no switch and under each: neither form every time, the same result."""
    out = []
    for on in ((), SWITCHES[:1], SWITCHES[1:]):
        _set(monkeypatch, on)
        out.append(call())
        assert _forms(sc) == (GENERIC, NONE), (what, on, _forms(sc))
    _set(monkeypatch)
    assert out[0].max() > 0 and all(np.array_equal(out[0], o) for o in out[1:]), what


def test_launches_that_are_generic_report_neither_form(gpu, dev_lib, monkeypatch):
    import torch
    data = _cornell()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)

    def default_frame():
        assert _frame(sc, monkeypatch)[2] == (PLAIN, DIFFUSE)  # (the records below are not left over from nothing)

    default_frame()
    _expect_generic(sc, monkeypatch, "jitter", lambda: sc.render(pixel_jitter=True, **KW))
    _expect_generic(sc, monkeypatch, "sample_lights off", lambda: sc.render(sample_lights=False, **KW))
    default_frame()
    px = np.stack([np.arange(0, 48, 3), np.arange(0, 48, 3) % cam.height], axis=1)
    _expect_generic(sc, monkeypatch, "render_samples", lambda: sc.render_samples(px, **KW))
    default_frame()

    def counting():
        d = torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda")
        sc.render_device(d.data_ptr(), None, count_work=True, **KW)
        torch.cuda.synchronize()
        assert sc.counters()["node_fetches"] > 0
        return d.cpu().numpy()

    _expect_generic(sc, monkeypatch, "count_work", counting)
    default_frame()
    rays = scenes.random_rays(200, *data.bounds(), seed=7)
    _expect_generic(sc, monkeypatch, "ray_color", lambda: sc.ray_color(rays, **KW))
    default_frame()
    _expect_generic(sc, monkeypatch, "fp32", lambda: sc.render(precision=F32, **KW))
    default_frame()  # (the fp32 tables change nothing for fp64)
    sc.close()


# ------------------------------------------------------------------------------------------------ 4
def test_the_flag_follows_the_material_table(gpu, dev_lib, monkeypatch):
    """No path changes a resident scene's materials (module docstring, 4): the flag is asserted on fresh uploads, alternating
    between a qualifying table and the same table with a mirror in one slot, inside one library."""
    plain = NOT_DIFFUSE["mirror-ball"]()
    a = api.Scene(_cornell()).upload(gpu)
    img_a, _, forms = _frame(a, monkeypatch)
    assert forms == (PLAIN, DIFFUSE)
    b = api.Scene(plain).upload(gpu)
    img_b, _, forms = _frame(b, monkeypatch)
    assert forms == (PLAIN, NONE)
    assert not np.array_equal(img_a, img_b)
    again, _, forms = _frame(a, monkeypatch)  # the flag is the scene's, not the library's last answer
    assert forms == (PLAIN, DIFFUSE) and np.array_equal(again, img_a)
    c = api.Scene(plain).upload(gpu)  # a fresh upload of the changed scene: the same frame
    img_c, _, forms = _frame(c, monkeypatch)
    assert forms == (PLAIN, NONE) and np.array_equal(img_c, img_b)
    for sc in (a, b, c):
        sc.close()


def test_the_shipped_library_knows_no_sub_form_and_reads_no_switch(gpu, monkeypatch):
    """libprt_hip.so: prt_last_render_subform answers UNKNOWN after a render, and PRT_TUNE_NO_DIFFUSE changes nothing it does."""
    sc = api.Scene(_cornell()).upload(gpu)
    assert sc._L.prt_dev_hooks() == 0
    a = sc.render(**KW)
    monkeypatch.setenv("PRT_TUNE_NO_DIFFUSE", "1")
    b = sc.render(**KW)
    assert api.last_render_subform(sc._L) == _abi.RENDER_SUBFORM_UNKNOWN
    assert np.array_equal(a, b)
    sc.close()
