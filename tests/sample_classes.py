"""Per-sample comparison of the fp32 fast mode with the oracle, by material class (numpy, CPU; used by
test_f32_samples_cpu.py, test_gpu_f32_samples.py and tools/f32_accounting.py).

The scenes are test_gpu_kernel_matrix.matrix_scene's: a Lambertian box with one small ball per special material.  A ball
covers 2-4 % of the frame, so a frame-level budget cannot see its material; here every SAMPLE is compared with the oracle's
sample of the same pixel, index and seed, and the samples are grouped by the materials their paths touch (the oracle's path
signature names the triangles).  A sample is CLOSE when every channel agrees to 1e-4 max(1, |x|): the rounding-only figure
of test_gpu_f32.check_image_tier2.  The fp32 arithmetic of a material that is right leaves nearly every sample of its class
close — the few that are not took another branch on a knife edge (a grazing hit, a roulette draw, a sampled lobe); one that
is off by more than 1e-4 leaves almost none of its class close.  The caps sit between the two:

    per class with at least MIN_CLASS samples   at most 5 % not close
    whole scene                                 at most 2 % not close (1 % at max_depth 0: first hit, light pick, shadow ray, Eval)

What they sit above is measured on the oracle alone (test_f32_samples_cpu.py): the eye moved by 16 fp32 ulps."""
import functools

import numpy as np

import oracle
from tests.test_gpu_kernel_matrix import _seed, matrix_scene

WIDTH, HEIGHT, SPP = 40, 32, 16
DEPTHS = (8, 0)
CASES = [(p, "quad") for p in ("lean", "tex", "phong", "ct", "all")] + [("lean", "sphere"), ("all", "sphere")]
CLOSE_REL = 1e-4
MIN_CLASS = 1000
CAP_CLASS = 0.05
CAP_SCENE = {8: 0.02, 0: 0.01}
EYE_SHIFT = 2.0 ** -18 * np.array([1.0, -0.7, 0.4])     # 16 fp32 ulps of a coordinate near 1


@functools.lru_cache(maxsize=None)
def scene(perm, lighting):
    return matrix_scene(perm, lighting, WIDTH, HEIGHT)


def pixels():
    return np.stack(np.meshgrid(np.arange(WIDTH), np.arange(HEIGHT)), -1).reshape(-1, 2)


def render_kw(perm, lighting, depth):
    return dict(max_depth=depth, seed=_seed(perm, lighting))


@functools.lru_cache(maxsize=None)
def oracle_samples(perm, lighting, depth, shifted=False):
    """The oracle's radiance (pixels, SPP, 3) and path signatures of every sample; shifted: the eye moved by EYE_SHIFT."""
    data = scene(perm, lighting)
    cam = data.camera
    if shifted:
        import dataclasses
        cam = dataclasses.replace(cam, eye=tuple(np.asarray(cam.eye) + EYE_SHIFT))
    orc = oracle.Oracle(data)
    out, tr = orc.render_samples(pixels(), camera=cam, spp=SPP, trace=True, **render_kw(perm, lighting, depth))
    orc.close()
    out.setflags(write=False)
    tr.setflags(write=False)
    return out, tr


def classes(data, trace):
    """{material name: (pixels, SPP) bool}: the samples whose path (the signature's vertices) touches that material."""
    tri_mat = np.repeat(np.asarray(data.mesh_material), np.diff(np.asarray(data.mesh_first_tri).astype(np.int64)))
    n_vert = trace[..., 0]
    prims = trace[..., 1::2][..., :int(n_vert.max())]
    valid = (np.arange(prims.shape[-1]) < n_vert[..., None]) & (prims >= 0)
    mats = np.where(valid, tri_mat[np.maximum(prims, 0)], -1)
    return {m.name: (mats == i).any(-1) for i, m in enumerate(data.materials)}


def rel_diff(x, ref):
    return (np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max(-1)


def shares(x, ref, cls):
    """{class or 'scene': {samples, not_close, close_median, close_max}} of samples x (pixels, SPP, 3) against ref."""
    rel = rel_diff(x, ref)
    close = rel <= CLOSE_REL
    out = {}
    for name, m in [("scene", np.ones_like(close))] + sorted(cls.items()):
        n = int(m.sum())
        c = rel[m & close]
        out[name] = {"samples": n, "not_close": float((m & ~close).sum() / n) if n else 0.0,
                     "close_median": float(np.median(c)) if c.size else 0.0, "close_max": float(c.max()) if c.size else 0.0}
    return out


def show(title, rep):
    print(f"\n{title}")
    for name, r in rep.items():
        print(f"  {name:10} {r['samples']:6d} samples, not close {100 * r['not_close']:6.3f} %, close: median {r['close_median']:.2e} "
              f"max {r['close_max']:.2e}")


def over_cap(rep, depth, factor=1.0):
    """The classes of a shares() report above their cap x factor: [(class, share, cap)] (empty: the conditions hold)."""
    bad = []
    for name, r in rep.items():
        cap = (CAP_SCENE[depth] if name == "scene" else CAP_CLASS) * factor
        if (name == "scene" or r["samples"] >= MIN_CLASS) and r["not_close"] > cap:
            bad.append((name, r["not_close"], cap))
    return bad
