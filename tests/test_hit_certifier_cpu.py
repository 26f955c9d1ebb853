"""CPU tests of tests/hit_certifier.py: a brute-force closest hit over all triangles, tri_test's expressions once in float64
(the oracle's role) and once in float32 operation by operation (the fp32 kernels' role), on edge-aimed rays.  Every
disagreement between the two must be certified as a rounding decision, same-primitive hits must stay inside the running
bound dt, and three planted faults — the mistakes the certifier exists to catch — must each be flagged."""
import functools

import numpy as np
import pytest

from pooraytracer_amd import scenes
from tests import hit_certifier as H

N = 10_000
SCENES = {"cornell": lambda: scenes.cornell_box(ball_subdiv=3), "mixed": lambda: scenes.mixed_materials(40, 40)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, rays, float64 hits, float32 hits, verdict), computed once per scene and left unchanged."""
    data = SCENES[name]()
    rays = H.edge_aimed_rays(data, N, seed=11)
    want = H.brute_force_closest(data.vertices, rays, np.float64)
    got = H.brute_force_closest(data.vertices, rays, np.float32)
    for a in (rays, want, got):
        a.setflags(write=False)
    return data, rays, want, got, H.certify(rays, want, got, data.vertices, H.U32)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_float32_disagreement_is_certified(name):
    data, rays, want, got, v = _case(name)
    print(f"\n{name}: {data.n_tris} triangles, {N} edge-aimed rays: {v.summary()}")
    assert v.unexplained.size == 0, (v.unexplained[:10], want[v.unexplained[:10]], got[v.unexplained[:10]])
    assert v.same_ratio <= 1.0 and v.ratio <= 1.0
    # the batch does what it is for: a few per cent of the rays decide differently in float32, in every way they can
    assert v.disagree >= 0.02 * N
    assert v.kinds["lost"] + v.kinds["farther"] > 0 and v.kinds["tie"] + v.kinds["nearer"] > 0 and v.kinds["phantom"] > 0
    finite = np.isfinite(rays["tmax"])
    assert 0.2 * N <= finite.sum() <= 0.3 * N


def test_the_batches_are_what_they_claim():
    data = SCENES["cornell"]()
    v = np.asarray(data.vertices)
    rays = H.edge_aimed_rays(data, 4000, seed=3)
    assert np.allclose(np.linalg.norm(rays["d"], axis=-1), 1.0, atol=1e-12)
    eye = (rays["o"] == np.asarray(data.camera.eye)).all(-1)
    assert 0.2 < eye.mean() < 0.3
    ax = H.axis_rays(data, 4000, seed=3)
    assert ((ax["d"] == 0).sum(-1) == 2).all() and (np.abs(ax["d"]).sum(-1) == 1).all()
    # an eighth of the targets are vertices: those drawn with delta = 0 (one in len(DELTAS)) are a vertex exactly
    tgt, extent = H._targets(data, 2000, np.random.default_rng(4))
    assert extent == (data.bounds()[1] - data.bounds()[0]).max()
    at_vertex = (tgt[:, None, None, :] == v[None]).all(-1).any((1, 2))
    assert at_vertex.sum() >= 0.5 * 2000 / 8 / len(H.DELTAS)
    big = H.scaled(data, 3e3)
    assert np.array_equal(big.vertices, v * 3e3) and big.camera.eye == tuple(3e3 * np.asarray(data.camera.eye))


def _robust_interior(data, rays, want, k=0.05):
    """Rays whose float64 hit lies well inside its triangle and its interval."""
    rec = H.tri_records(data.vertices)
    hit = want["prim"] >= 0
    E = {key: np.full(rays.shape[0], np.nan) for key in ("alpha", "beta", "t", "nd")}
    for key, val in H.evaluate(rec, want["prim"][hit], rays["o"][hit], rays["d"][hit], H.U32).items():
        if key in E:
            E[key][hit] = val
    with np.errstate(invalid="ignore"):
        return hit & (E["alpha"] > k) & (E["beta"] > k) & (E["alpha"] + E["beta"] < 1 - k) & (E["nd"] > 0.05) & \
            (E["t"] > 2 * rays["tmin"]) & (E["t"] < 0.5 * rays["tmax"])


def test_planted_faults_are_flagged():
    """The certifier must not explain: a triangle the float32 pass never tests, a hit moved by 1e-3 of its distance, a robust
    interior hit reported as a miss.  Interior rays come from a random batch (edge-aimed rays rarely have one)."""
    data = SCENES["cornell"]()
    lo, hi = data.bounds()
    rays = scenes.random_rays(3000, lo, hi, seed=5)
    want = H.brute_force_closest(data.vertices, rays, np.float64)
    got = H.brute_force_closest(data.vertices, rays, np.float32)
    assert H.certify(rays, want, got, data.vertices, H.U32).unexplained.size == 0
    robust = _robust_interior(data, rays, want)
    assert robust.sum() > 300

    # 1. a dropped triangle: every robust hit of it must be flagged (the float32 pass returns what lies behind, or nothing)
    drop = np.bincount(want["prim"][robust]).argmax()
    v = H.certify(rays, want, H.brute_force_closest(data.vertices, rays, np.float32, drop=drop), data.vertices, H.U32)
    victims = np.flatnonzero(robust & (want["prim"] == drop))
    assert victims.size > 0 and np.isin(victims, v.unexplained).all()
    assert np.isin(v.unexplained, np.flatnonzero(want["prim"] == drop)).all()   # and nothing else is

    # 2. one hit moved to t (1 + 1e-3), same primitive
    i = np.flatnonzero(robust)[7]
    moved = got.copy()
    moved["t"][i] *= 1.0 + 1e-3
    assert H.certify(rays, want, moved, data.vertices, H.U32).unexplained.tolist() == [i]

    # 3. one robust interior hit replaced by a miss
    j = np.flatnonzero(robust)[11]
    missed = got.copy()
    missed["prim"][j], missed["t"][j] = -1, rays["tmax"][j]
    assert H.certify(rays, want, missed, data.vertices, H.U32).unexplained.tolist() == [j]

    # and a robust hit of another primitive behind the true one is flagged, too (X is a hit, but Y was not marginal)
    far = got.copy()
    k = np.flatnonzero(robust & (want["prim"] != want["prim"][i]))[0]
    far["prim"][k], far["t"][k] = want["prim"][i], want["t"][k] * 1.5
    assert k in H.certify(rays, want, far, data.vertices, H.U32).unexplained


def test_fp64_roundoff_certifies_float64_against_long_double():
    """u = 2^-53: the float64 brute force against a long-double one (the certifier evaluates above the kernel's precision)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double on this platform")
    data = SCENES["mixed"]()
    rays = H.edge_aimed_rays(data, 2000, seed=12)
    want = H.brute_force_closest(data.vertices, rays, np.longdouble)
    got = H.brute_force_closest(data.vertices, rays, np.float64)
    v = H.certify(rays, want, got, data.vertices, H.U64)
    print(v.summary())
    assert v.unexplained.size == 0 and v.same_ratio <= 1.0
