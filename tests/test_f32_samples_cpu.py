"""CPU test of the precondition of test_gpu_f32_samples.py: what the caps of tests/sample_classes.py sit above.

The oracle against itself with the eye moved by 2^-18 (1, -0.7, 0.4) — 16 fp32 ulps, far more than the fp32 kernels' own
input rounding — on the same scenes, seeds and depths: the share of samples that leave the 1e-4 closeness is the
conditioning of the scenes themselves (samples whose path sits on a knife edge), the floor under any fp32 implementation.
It must stay at or below HALF of each cap, so that a cap can only be crossed by an error of the kernels, and so that a change
of the scenes that moves this floor is noticed here, without a GPU."""
import pytest

from tests import sample_classes as S


@pytest.mark.parametrize("depth", S.DEPTHS)
@pytest.mark.parametrize("perm,lighting", S.CASES)
def test_the_reference_alone_moves_less_than_half_of_each_cap(perm, lighting, depth):
    data = S.scene(perm, lighting)
    ref, trace = S.oracle_samples(perm, lighting, depth)
    moved, _ = S.oracle_samples(perm, lighting, depth, shifted=True)
    cls = S.classes(data, trace)
    rep = S.shares(moved, ref, cls)
    S.show(f"{perm}/{lighting} depth {depth}: oracle with the eye moved by 2^-18 against the oracle", rep)
    assert S.over_cap(rep, depth, factor=0.5) == []
    # the classes are what the test is about: every special material of the scene has a class large enough to be held to its cap
    special = [m.name for m in data.materials if m.name not in ("White", "Red", "Green", "Light")]
    assert special and all(rep[name]["samples"] >= S.MIN_CLASS for name in special), {n: rep[n]["samples"] for n in special}


def test_classes_follow_the_path_signature():
    data = S.scene("all", "quad")
    _, trace = S.oracle_samples("all", "quad", 0)
    cls = S.classes(data, trace)
    # depth 0: one vertex per sample, so the classes partition the samples that hit something
    total = sum(m.astype(int) for m in cls.values())
    assert total.max() == 1 and (total == (trace[..., 1] >= 0)).all() and (trace[..., 0] == 1).all()
    _, deep = S.oracle_samples("all", "quad", 8)
    assert sum(m.astype(int) for m in S.classes(data, deep).values()).max() > 1
