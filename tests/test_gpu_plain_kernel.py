"""The PLAIN form of the render kernel K3 (-m gpu).  A frame with default settings — no pixel jitter, the
owned tiles as items, light sampling on, a scene with emitters whose light triangles are all staged in LDS, no counting, no
ray batch — launches k_render<false, FEAT | PRT_FEAT_PLAIN, true, PAD>, in which those launch-uniform conditions are
constants; every other launch, and every launch under the dev-hooks library's PRT_TUNE_GENERIC=1, keeps the generic kernel.
The dev-hooks library says which form its last launch used (prt_last_render_form).

  1. PLAIN equals generic, bit for bit: the framebuffer and both ray counts, on five scenes with host-built and device-built
     trees, on a tile share, with padded triangle records, and in fp32.  Each case asserts that its first launch was PLAIN and
     its second generic.
  2. Launches that must not be PLAIN are reported as generic, with and without the forcing switch (and give the same frame).

All frames are 40 x 32 or smaller, spp 6, depth 6, seed 1.  mixed_materials() is rendered through a 40 x 32 camera at its
own viewpoint (its default frame is 48 x 48).

Two of the five scenes do not launch a PLAIN kernel, and their cases below assert GENERIC for both launches — they pin the
selection and the harmlessness of the switch, not the equality of two kernels:
  * veach_mis: its five sphere lights are 400 triangles at light_subdiv=1 (6400 in the benchmark's scene); light triangles
    are staged in LDS only up to 32 of them, so its launches do not meet the fifth condition of PLAIN (the rule of case 2,
    `light triangles not in LDS`);
  * bathroom: the textured permutation keeps its generic kernel (its PLAIN form gave the same bits and measured 1.4 % slower
    on bathroom2); mixed_materials covers textures in a PLAIN kernel (the permutation with everything).
No fp32 permutation has a PLAIN form (bit-identical where tried, none faster): every fp32 launch is reported as generic.
"""
import dataclasses

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, distributed, scenes

pytestmark = pytest.mark.gpu
F64, F32 = _abi.PRECISION_F64, _abi.PRECISION_F32
PLAIN, GENERIC = _abi.RENDER_FORM_PLAIN, _abi.RENDER_FORM_GENERIC
KW = dict(spp=6, max_depth=6, seed=1)

SCENES = {
    "cornell": lambda: scenes.cornell_box(ball_subdiv=1, width=40, height=32),
    "cornell-ct": lambda: scenes.cornell_box(ball_subdiv=1, width=40, height=32, ball_cooktorrance_alpha=0.1),
    "veach-mis": lambda: scenes.veach_mis(width=40, height=24, light_subdiv=1, plate_cells=2),
    "bathroom": lambda: scenes.bathroom(width=40, height=24, detail=0.15),
    "mixed": lambda: scenes.mixed_materials(),
}
# the form of a default frame (module docstring: veach-mis, bathroom)
FORM = {"cornell": PLAIN, "cornell-ct": PLAIN, "veach-mis": GENERIC, "bathroom": GENERIC, "mixed": PLAIN}
# ... and of a default fp32 frame: the fp32 translation unit has no PLAIN form
FORM_F32 = {"cornell": GENERIC, "cornell-ct": GENERIC, "veach-mis": GENERIC, "bathroom": GENERIC, "mixed": GENERIC}
_DATA = {}


def _data(name):
    if name not in _DATA:
        _DATA[name] = SCENES[name]()
    return _DATA[name]


def _camera(data):
    cam = data.camera
    return cam if cam.width <= 40 and cam.height <= 32 else dataclasses.replace(cam, width=40, height=32)


def _form(sc):
    return api.last_render_form(sc._L)


def _frame(sc, monkeypatch, forced, **kw):
    """One frame, its ray counts and the form of its launch; `forced`: under PRT_TUNE_GENERIC=1."""
    if forced:
        monkeypatch.setenv("PRT_TUNE_GENERIC", "1")
    else:
        monkeypatch.delenv("PRT_TUNE_GENERIC", raising=False)
    img = sc.render(camera=_camera(sc.data), **KW, **kw)
    cnt = sc.counters()
    monkeypatch.delenv("PRT_TUNE_GENERIC", raising=False)
    return img, (cnt["rays_closest"], cnt["rays_shadow"]), _form(sc)


def _assert_both_forms_agree(sc, monkeypatch, first, where, **kw):
    """The frame as launched and under the forcing switch: the forms `first` and GENERIC, the same bits, the same rays."""
    a, rays_a, form_a = _frame(sc, monkeypatch, False, **kw)
    b, rays_b, form_b = _frame(sc, monkeypatch, True, **kw)
    assert form_a == first, where
    assert form_b == GENERIC, where
    assert a.max() > 0 and rays_a[0] > 0, where
    assert np.array_equal(a, b), (where, int((a != b).sum()))
    assert rays_a == rays_b, where
    return a


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("device_bvh", [False, True], ids=["host-tree", "device-tree"])
@pytest.mark.parametrize("name", list(SCENES))
def test_plain_frame_equals_generic_frame(gpu, dev_lib, monkeypatch, name, device_bvh):
    assert dev_lib.prt_dev_hooks() == 1
    sc = api.Scene(_data(name), device_bvh=device_bvh).upload(gpu)
    _assert_both_forms_agree(sc, monkeypatch, FORM[name], (name, device_bvh))
    sc.close()


@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_plain_equals_generic_on_a_tile_share(gpu, dev_lib, monkeypatch, name):
    sc = api.Scene(_data(name)).upload(gpu)
    share = dict(rank=1, nranks=3, tile_size=16)
    img = _assert_both_forms_agree(sc, monkeypatch, PLAIN, (name, "share"), **share)
    own = distributed.owned_mask(40, 32, share["tile_size"], share["rank"], share["nranks"])
    assert 0 < own.sum() < own.size and img[own].any() and not img[~own].any()
    sc.close()


@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_plain_equals_generic_with_padded_records(gpu, dev_lib, monkeypatch, name):
    monkeypatch.setenv("PRT_TUNE_TRI_STRIDE", "128")
    sc = api.Scene(_data(name)).upload(gpu)
    monkeypatch.delenv("PRT_TUNE_TRI_STRIDE")
    info = sc.bvh_info()
    assert info["tri_stride"] == 128 and info["render_variant"] & _abi.VARIANT_PAD
    _assert_both_forms_agree(sc, monkeypatch, PLAIN, (name, "padded"))
    sc.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_fp32_frames_agree_under_the_switch(gpu, dev_lib, monkeypatch, name):
    """fp32 (FORM_F32: no permutation has a PLAIN form there): a launch reports the form it used, the switch changes no bit;
    and an fp64 frame of the same scene afterwards is launched as before."""
    sc = api.Scene(_data(name)).upload(gpu)
    _assert_both_forms_agree(sc, monkeypatch, FORM_F32[name], (name, "f32"), precision=F32)
    _assert_both_forms_agree(sc, monkeypatch, FORM[name], (name, "f64 after f32"))  # (the fp32 tables change nothing for fp64)
    sc.close()


# ------------------------------------------------------------------------------------------------ 2
def _without_emitters(data):
    keep = [i for i, m in enumerate(data.mesh_material) if data.materials[int(m)].type != _abi.MAT_DIFFUSE_LIGHT]
    first = data.mesh_first_tri.astype(np.int64)
    tris = np.concatenate([np.arange(first[i], first[i + 1]) for i in keep])
    sizes = [int(first[i + 1] - first[i]) for i in keep]
    return dataclasses.replace(data, name=data.name + "-dark", vertices=data.vertices[tris], texcoords=data.texcoords[tris],
                               normals=data.normals[tris], mesh_first_tri=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64),
                               mesh_material=data.mesh_material[keep], mesh_names=[data.mesh_names[i] for i in keep])


@pytest.mark.parametrize("case", ["jitter", "sample_lights_off", "no_emitter", "ltri_lds_off"])
def test_frames_that_must_not_be_plain_are_generic(gpu, dev_lib, monkeypatch, case):
    data = _data("cornell")
    kw = {}
    if case == "jitter":
        kw = dict(pixel_jitter=True)
    elif case == "sample_lights_off":
        kw = dict(sample_lights=False)
    elif case == "no_emitter":
        data, kw = _without_emitters(data), dict(background=(0.3, 0.4, 0.5))
    elif case == "ltri_lds_off":
        monkeypatch.setenv("PRT_TUNE_LTRI_LDS", "0")
    sc = api.Scene(data).upload(gpu)
    monkeypatch.delenv("PRT_TUNE_LTRI_LDS", raising=False)
    if case == "ltri_lds_off":
        info = sc.bvh_info()
        assert info["lds_light_tris"] == 0 and info["lds_materials"] > 0  # (still an LLDS kernel: the other tables stay)
    _assert_both_forms_agree(sc, monkeypatch, GENERIC, case, **kw)
    if case in ("jitter", "sample_lights_off"):  # the same scene's default frame is PLAIN: the launch decides, not the scene
        _assert_both_forms_agree(sc, monkeypatch, PLAIN, (case, "default frame"))
    sc.close()


def _forced(monkeypatch, on):
    if on:
        monkeypatch.setenv("PRT_TUNE_GENERIC", "1")
    else:
        monkeypatch.delenv("PRT_TUNE_GENERIC", raising=False)


def test_render_samples_counting_runs_and_ray_batches_are_generic(gpu, dev_lib, monkeypatch):
    import torch
    data = _data("cornell")
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    _assert_both_forms_agree(sc, monkeypatch, PLAIN, "default frame")  # (the record below is not left over from nothing)
    # prt_render_samples on a pixel list
    px = np.stack([np.arange(0, 40, 3), np.arange(0, 40, 3) % cam.height], axis=1)
    out = []
    for on in (False, True):
        _forced(monkeypatch, on)
        out.append(sc.render_samples(px, **KW))
        assert _form(sc) == GENERIC, ("render_samples", on)
    assert out[0].max() > 0 and np.array_equal(out[0], out[1])
    # a counting run
    out = []
    for on in (False, True):
        _forced(monkeypatch, on)
        d = torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda")
        sc.render_device(d.data_ptr(), None, count_work=True, **KW)
        torch.cuda.synchronize()
        assert _form(sc) == GENERIC, ("count_work", on)
        cnt = sc.counters()
        assert cnt["node_fetches"] > 0
        out.append((d.cpu().numpy(), cnt["rays_closest"], cnt["rays_shadow"], cnt["node_fetches"], cnt["tri_tests"]))
    assert out[0][0].max() > 0 and np.array_equal(out[0][0], out[1][0]) and out[0][1:] == out[1][1:]
    _forced(monkeypatch, False)
    assert _frame(sc, monkeypatch, False)[2] == PLAIN
    # prt_ray_color
    rays = scenes.random_rays(200, *data.bounds(), seed=7)
    out = []
    for on in (False, True):
        _forced(monkeypatch, on)
        out.append(sc.ray_color(rays, **KW))
        assert _form(sc) == GENERIC, ("ray_color", on)
    assert out[0].max() > 0 and np.array_equal(out[0], out[1])
    _forced(monkeypatch, False)
    sc.close()


def test_the_shipped_library_keeps_no_record_and_reads_no_switch(gpu, monkeypatch):
    """libprt_hip.so: prt_last_render_form answers UNKNOWN after a render, and PRT_TUNE_GENERIC changes nothing it does."""
    sc = api.Scene(_data("cornell")).upload(gpu)
    assert sc._L.prt_dev_hooks() == 0
    a = sc.render(**KW)
    monkeypatch.setenv("PRT_TUNE_GENERIC", "1")
    b = sc.render(**KW)
    assert api.last_render_form(sc._L) == _abi.RENDER_FORM_UNKNOWN
    assert np.array_equal(a, b)
    sc.close()
