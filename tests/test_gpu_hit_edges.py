"""GPU tests (-m gpu) of the ray-batch kernels on rays aimed where they go wrong: triangle edges and vertices, interval
ends, axis-parallel rays inside box faces and through box corners (tests/hit_certifier.py makes the batches).

Every hit of every batch goes through the certifier with the oracle's closest hit: a ray on which kernel and oracle
disagree must be within a rounding bound of the decision taken the other way — ZERO unexplained rays, in fp32 (u = 2^-24)
as in fp64 (u = 2^-53), on host- and device-built trees, packed and padded records.  A lost robust hit (a slab pad that is
too small, a stack entry dropped in the fp32 kernels' 32-entry collapse, a wrong update of the running tmax) is exactly
what no rounding explains.  On the same batches the exact contracts of the query family: the any-hit byte is (prim >= 0)
of the closest-hit call, bytes 0-31 of the surface record are its PrtHit, and the sorted call equals the plain one."""
import functools

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, scenes
from tests import hit_certifier as H
from tests.test_gpu_occlusion import _closest, _dev, _occluded
from tests.test_gpu_surface import _head_bytes, _hit_bytes, _surface

pytestmark = pytest.mark.gpu

SCENES = {
    "cornell": lambda: scenes.cornell_box(ball_subdiv=3),
    "mixed": lambda: scenes.mixed_materials(40, 40),
    # the smallest soup of the suite whose 4-wide tree needs the fp32 kernels' second, shallower collapse
    "soup": lambda: scenes.triangle_soup(n_tris=150_000, seed=5),
    "cornell-x1e-4": lambda: H.scaled(scenes.cornell_box(ball_subdiv=3), 1e-4),
    "cornell-x3e3": lambda: H.scaled(scenes.cornell_box(ball_subdiv=3), 3e3),
}
N_EDGE, N_AXIS = 24_000, 20_000     # 23.4 and 19.5 x PRT_K1_CHUNK (1024 rays): many refills per wave, a ragged last chunk
PRECISIONS = ((_abi.PRECISION_F64, H.U64, "f64"), (_abi.PRECISION_F32, H.U32, "f32"))
assert N_EDGE % 1024 and N_AXIS % 1024


@functools.lru_cache(maxsize=None)
def batches(name):
    """(scene, ((family, rays, the oracle's closest hits), ...)), computed once per scene and left unchanged."""
    data = SCENES[name]()
    orc = oracle.Oracle(data)
    out = []
    for family, rays in (("edge", H.edge_aimed_rays(data, N_EDGE, seed=41)), ("axis", H.axis_rays(data, N_AXIS, seed=42))):
        want = orc.trace_closest(rays)
        for a in (rays, want):
            a.setflags(write=False)
        out.append((family, rays, want))
    orc.close()
    return data, tuple(out)


def check_case(sc, name, where=""):
    """Every batch of scene `name` on the uploaded scene `sc`, both precisions: the certifier and the exact contracts.
    Returns {(family, precision): Verdict.summary()} (tools/f32_accounting.py records it)."""
    data, families = batches(name)
    report = {}
    for family, rays, want in families:
        d_r = _dev(rays)
        for prec, u, pname in PRECISIONS:
            plain = _closest(sc, rays, precision=prec, d_r=d_r)
            v = H.certify(rays, want, plain, data.vertices, u)
            s = v.summary()
            s["hit_share"] = float((plain["prim"] >= 0).mean())
            print(f"{name}{where} {family} {pname}: {rays.shape[0]} rays, {s}")
            bad = v.unexplained[:8]
            assert v.unexplained.size == 0, (name, family, pname, bad.tolist(), rays[bad], want[bad], plain[bad])
            assert v.ratio < 1.0                       # the worst explained margin, in units of its bound
            assert (v.ratio_of[(plain["prim"] == want["prim"])] <= 1.0).all()   # the same-primitive bound, on every ray
            report[(family, pname)] = s
            # ---- the exact contracts, plain and sorted
            for sort in (False, True):
                hits = _closest(sc, rays, precision=prec, sort=sort, d_r=d_r)
                assert np.array_equal(_hit_bytes(hits), _hit_bytes(plain)), (name, family, pname, "sorted closest hit")
                occ = _occluded(sc, rays, precision=prec, sort=sort, d_r=d_r)
                mism = np.flatnonzero(occ.astype(bool) != (plain["prim"] >= 0))
                assert set(np.unique(occ)) <= {0, 1} and mism.size == 0, (name, family, pname, sort, mism[:8].tolist(), rays[mism[:8]])
                heads = _head_bytes(_surface(sc, rays, precision=prec, sort=sort, d_r=d_r))
                diff = np.flatnonzero((heads != _hit_bytes(plain)).any(1))
                assert diff.size == 0, (name, family, pname, sort, diff[:8].tolist(), rays[diff[:8]])
            # ---- guards against an empty test
            if family == "edge" and prec == _abi.PRECISION_F32:
                assert v.disagree >= 0.02 * rays.shape[0], s
            if family == "axis":
                assert s["hit_share"] >= 0.25, s
    return report


@pytest.mark.parametrize("device_bvh", [False, True], ids=["host-bvh", "device-bvh"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_disagreement_with_the_oracle_is_certified(gpu, name, device_bvh):
    sc = api.Scene(batches(name)[0], device_bvh=device_bvh).upload(gpu)
    print(f"{name}: {sc.bvh_info()['n_nodes']} nodes, stack need {sc.bvh_info()['stack_need']}")
    check_case(sc, name, where=f" device_bvh={device_bvh}")
    sc.close()


def test_padded_records(gpu, dev_lib, monkeypatch):
    """The PAD instantiations (one record per cache line: 128 bytes in fp64, 64 in fp32) on the edge batches."""
    monkeypatch.setenv("PRT_TUNE_TRI_STRIDE", "128")
    sc = api.Scene(batches("mixed")[0]).upload(gpu)
    assert sc.bvh_info()["tri_stride"] == 128
    check_case(sc, "mixed", where=" padded")
    sc.close()
