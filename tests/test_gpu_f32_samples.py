"""GPU tests (-m gpu) of the fp32 fast mode's shading, sample by sample (tests/sample_classes.py has the scenes, the
classes and the caps).

No hook is needed to see an fp32 sample: an Accumulator in fp32 renders in fp32 and sums in fp64, so sixteen add(1) passes
with state() after each give every sample of every pixel as a difference of consecutive sums.  In fp64 mode the same
reconstruction must be Scene.render_samples to 1e-12, which validates it.  Every fp32 sample is then held against the
oracle's sample of the same pixel, index and seed; per material class and per scene the share that is not close (1e-4) must
stay under the caps, at max_depth 8 and at max_depth 0 (first hit, light pick, shadow ray, Eval alone).  Last, what only
multi-sample passes run — the cached primary hit, the one-pass vertex, the sample turnover inside a pass: one add(16) pass
must be the sum of the sixteen single passes, to the rounding of an fp32 sum of sixteen terms."""
import functools

import numpy as np
import pytest

from pooraytracer_amd import _abi, api
from tests import sample_classes as S

pytestmark = pytest.mark.gpu
F64, F32 = _abi.PRECISION_F64, _abi.PRECISION_F32


def accumulator_samples(sc, precision, **kw):
    """((pixels, SPP, 3) samples from SPP passes of one sample each, [(pixels, 3) sums of ONE pass of SPP samples: as one work
    item per pixel (sample_chunks=1: all sixteen samples run through one lane's sample turnover), and chunked as the library
    chooses (on a frame this small: sixteen items of one sample)])."""
    with api.Accumulator(sc, precision=precision, **kw) as acc:
        sums = [np.zeros((S.HEIGHT, S.WIDTH, 3))]
        for k in range(S.SPP):
            acc.add(1)
            s, n, _ = acc.state()
            assert n == k + 1
            sums.append(s)
    one_pass = []
    for chunks in (1, 0):
        with api.Accumulator(sc, precision=precision, sample_chunks=chunks, **kw) as acc:
            acc.add(S.SPP)
            total, n, _ = acc.state()
            assert n == S.SPP
            one_pass.append(total.reshape(-1, 3))
    samples = np.diff(np.stack(sums), axis=0)                      # (SPP, H, W, 3)
    return samples.reshape(S.SPP, -1, 3).transpose(1, 0, 2), one_pass


@functools.lru_cache(maxsize=None)
def gpu_samples(perm, lighting, depth, precision):
    sc = api.Scene(S.scene(perm, lighting)).upload(0)
    out = accumulator_samples(sc, precision, **S.render_kw(perm, lighting, depth))
    sc.close()
    for a in [out[0]] + out[1]:
        a.setflags(write=False)
    return out


def class_report(perm, lighting, depth):
    """shares() of the fp32 samples against the oracle's, by the classes of the oracle's paths."""
    ref, trace = S.oracle_samples(perm, lighting, depth)
    got, _ = gpu_samples(perm, lighting, depth, F32)
    assert np.isfinite(got).all()
    return S.shares(got, ref, S.classes(S.scene(perm, lighting), trace))


@pytest.mark.parametrize("depth", S.DEPTHS)
def test_the_reconstruction_is_render_samples_in_fp64(gpu, depth):
    """Differences of consecutive fp64 sums are the samples prt_render_samples returns (which test_gpu_parity.py and
    test_gpu_kernel_matrix.py hold against the oracle per sample), and the oracle's."""
    perm, lighting = "all", "sphere"
    got, _ = gpu_samples(perm, lighting, depth, F64)
    sc = api.Scene(S.scene(perm, lighting)).upload(gpu)
    want = sc.render_samples(S.pixels(), spp=S.SPP, **S.render_kw(perm, lighting, depth))
    sc.close()
    # a difference of sums carries the rounding of the sums: 1e-12 of the larger of the sample and the running sum
    scale = np.maximum(1.0, np.maximum(np.abs(want), np.cumsum(np.abs(want), axis=1)))
    assert (np.abs(got - want) <= 1e-12 * scale).all(), float((np.abs(got - want) / scale).max())
    ref, _ = S.oracle_samples(perm, lighting, depth)
    assert (S.rel_diff(want, ref) <= 1e-9).all()
    assert (np.abs(want).sum(-1) > 0).mean() > 0.05       # (not a comparison of zeros: the small sphere light leaves most depth-0 samples black)


@pytest.mark.parametrize("depth", S.DEPTHS)
@pytest.mark.parametrize("perm,lighting", S.CASES)
def test_fp32_samples_by_material_class(gpu, perm, lighting, depth):
    rep = class_report(perm, lighting, depth)
    S.show(f"{perm}/{lighting} depth {depth}: fp32 samples against the oracle's", rep)
    assert S.over_cap(rep, depth) == []


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("depth", S.DEPTHS)
@pytest.mark.parametrize("perm,lighting", S.CASES)
def test_one_pass_of_sixteen_is_the_sum_of_sixteen_passes(gpu, perm, lighting, depth, precision):
    samples, one_pass = gpu_samples(perm, lighting, depth, precision)
    total, mag = samples.sum(1), np.abs(samples).sum(1)
    # fp32: a pass sums its samples in fp32, in an order of its own: 16 roundings of at most 2^-24 of the terms' magnitude
    bound = (S.SPP * 2.0 ** -24 if precision == F32 else 1e-13) * mag
    for name, sums in zip(("one item per pixel", "library's chunks"), one_pass):
        gap = np.abs(sums - total)
        worst = float((gap / np.maximum(bound, 1e-300)).max())
        print(f"{perm}/{lighting} depth {depth} precision {precision}, {name}: largest gap / bound {worst:.3e}")
        assert (gap <= bound).all(), (name, worst)
