"""GPU tests (-m gpu) of the multi-hit queries (prt_trace_multi*, Scene.trace_multi*, Hittable::Hits; K7, multi_hit.hip).

Every list of every batch goes through the list certifier of tests/multi_hit_model.py - ZERO unexplained rays in fp64
(u = 2^-53) as in fp32 (u = 2^-24), on host- and device-built trees, packed and padded records, after a refit - and the
exact contracts are checked as byte equalities: the lists do not depend on the tree, the batch order or count_work; pages
fed their predecessor's last record are the one call; exact ties come in ascending prim."""
import os
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, build, scenes
from tests import hit_certifier as H
from tests import multi_hit_model as M

pytestmark = pytest.mark.gpu

PRECISIONS = ((_abi.PRECISION_F64, H.U64, "f64"), (_abi.PRECISION_F32, H.U32, "f32"))
KS = (1, 3, 8)
FILL = -1.2345e300  # what an output buffer holds before a call


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float64).reshape(a.shape[0], a.dtype.itemsize // 8).copy()).cuda()


def _multi(sc, rays, k, precision=0, sort=False, count_work=False, after=None, d_r=None, guard=0, stream=None, sync=True):
    """The (n, k) lists (and, with `guard`, the records behind them of a buffer prefilled with FILL)."""
    import torch
    n = rays.shape[0]
    d_r = _dev(rays) if d_r is None else d_r
    d_a = None if after is None else _dev(after)
    d_h = torch.full((max(n * k, 1) + guard, 4), FILL, dtype=torch.float64, device="cuda")
    sc.trace_multi_device(d_r.data_ptr(), n, k, d_h.data_ptr(), None if d_a is None else d_a.data_ptr(), count_work=count_work,
                          precision=precision, sort=sort, stream=stream)
    if not sync:
        return d_h, (d_r, d_a)
    torch.cuda.synchronize()
    out = d_h.cpu().numpy()
    lists = out[:n * k].view(_abi.HIT_DTYPE).reshape(n, k)
    return (lists, out[n * k:]) if guard else lists


def _bytes(lists):
    return np.ascontiguousarray(lists).view(np.uint8).reshape(lists.shape[0], -1)


def _variants(rays):
    return (("as generated", rays), ("whole line", M.whole_line(rays)))


def check_case(sc, name, where=""):
    """Every batch of scene `name` on the uploaded scene `sc`: as generated and over the whole line, k = 1, 3, 8, both
    precisions, certified against the model."""
    for family, rays, _ in M.batches(name):
        for which, batch in _variants(rays):
            d_r = _dev(batch)
            for prec, u, pname in PRECISIONS:
                cert = M.certifier(name, family, u)
                for k in KS:
                    got = _multi(sc, batch, k, precision=prec, d_r=d_r)
                    v = cert.certify(batch, got)
                    print(f"{name}{where} {family} {which} {pname} k={k}: {batch.shape[0]} rays, {v.summary()}")
                    bad = v.unexplained[:6]
                    assert v.unexplained.size == 0, (name, family, which, pname, k, v.summary(), bad.tolist(), batch[bad], got[bad])
                    assert v.worst_entry < 1.0 and v.entries > 0


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("device_bvh", [False, True], ids=["host-bvh", "device-bvh"])
@pytest.mark.parametrize("name", sorted(M.SCENES))
def test_every_list_is_certified(gpu, name, device_bvh):
    sc = api.Scene(M.scene(name), device_bvh=device_bvh).upload(gpu)
    print(f"{name}: {sc.bvh_info()['n_nodes']} nodes, stack need {sc.bvh_info()['stack_need']}")
    check_case(sc, name, where=f" device_bvh={device_bvh}")
    sc.close()


# ------------------------------------------------------------------------------------------------ 2
def test_exact_ties_come_in_ascending_prim(gpu):
    """The stack's quad 3 (triangles 6, 7) has three bit-identical copies (64..69): a ray through it reports a run of four
    equal t in ascending prim, in either precision, and every run of equal t anywhere ascends in prim."""
    data = M.scene("stack")
    _, rays, pr = M.batches("stack")[0]
    model = M.model_hits(data.vertices, rays, np.float64, 8, pr=pr)[0]
    model_tie = ((model["t"][:, 1:] == model["t"][:, :-1]) & (model["prim"][:, 1:] >= 0)).any(1)
    sc = api.Scene(data).upload(gpu)
    for prec, _, pname in PRECISIONS:
        got = _multi(sc, rays, 8, precision=prec)
        t, p = got["t"], got["prim"]
        tie = (t[:, 1:] == t[:, :-1]) & (p[:, 1:] >= 0)
        assert (p[:, 1:][tie] > p[:, :-1][tie]).all()
        runs = 0
        for a, copies in ((6, (64, 66, 68)), (7, (65, 67, 69))):
            r, c = np.nonzero((p == a) & (np.arange(8)[None, :] <= 4))
            for j, q in enumerate(copies, 1):
                assert np.array_equal(p[r, c + j], np.full(r.size, q)) and np.array_equal(t[r, c + j], t[r, c])
            runs += r.size
        both = model_tie & tie.any(1)
        print(f"stack {pname}: {tie.any(1).mean():.3f} of the rays report an exact tie, {runs} runs of four, "
              f"{both.sum()} of the model's {model_tie.sum()} tie rays among them")
        assert runs > 0.05 * rays.shape[0]
        dup = model_tie & np.isin(model["prim"], (6, 7)).any(1)  # a model tie made by the copies is a kernel tie as well
        assert dup.sum() > 0.05 * rays.shape[0] and tie.any(1)[dup & np.isin(p[:, :5], (6, 7)).any(1)].all()
    sc.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", sorted(M.SCENES))
def test_bytes_do_not_depend_on_tree_order_or_counting(gpu, name):
    data = M.scene(name)
    host = api.Scene(data).upload(gpu)
    dev = api.Scene(data, device_bvh=True).upload(gpu)
    ref = {}
    for family, rays, _ in M.batches(name):
        d_r = _dev(rays)
        for prec, _, pname in PRECISIONS:
            for k in (3, 8):
                want = _bytes(_multi(host, rays, k, precision=prec, d_r=d_r))
                ref[(family, pname, k)] = want
                for what, sc, kw in (("host sorted", host, dict(sort=True)), ("host counting", host, dict(count_work=True)),
                                     ("device", dev, {}), ("device sorted counting", dev, dict(sort=True, count_work=True))):
                    got = _bytes(_multi(sc, rays, k, precision=prec, d_r=d_r, **kw))
                    diff = np.flatnonzero((got != want).any(1))
                    assert diff.size == 0, (name, family, pname, k, what, diff[:6].tolist(), rays[diff[:6]])
    host.rebuild(np.ascontiguousarray(data.vertices, dtype=np.float64))  # a new tree of the same vertices
    for family, rays, _ in M.batches(name):
        for prec, _, pname in PRECISIONS:
            got = _bytes(_multi(host, rays, 8, precision=prec))
            diff = np.flatnonzero((got != ref[(family, pname, 8)]).any(1))
            assert diff.size == 0, (name, family, pname, "rebuilt", diff[:6].tolist())
    host.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", ["stack", "mixed"])
def test_pages_are_the_one_call(gpu, name):
    sc = api.Scene(M.scene(name)).upload(gpu)
    for family, rays, _ in M.batches(name)[:2]:
        for which, batch in _variants(rays):
            d_r = _dev(batch)
            for prec, _, pname in PRECISIONS:
                one = _multi(sc, batch, 8, precision=prec, d_r=d_r)
                for k1 in (2, 1):
                    cur, pages = None, []
                    for _ in range(8 // k1):
                        page = _multi(sc, batch, k1, precision=prec, after=cur, d_r=d_r)
                        pages.append(page)
                        cur = M.next_cursors(page, cur)
                    got = np.concatenate(pages, 1)
                    diff = np.flatnonzero((_bytes(got) != _bytes(one)).any(1))
                    assert diff.size == 0, (name, family, which, pname, k1, diff[:6].tolist(), got[diff[:6]], one[diff[:6]])
                # a further page after the last hit is all misses
                cur, total = None, np.zeros(batch.shape[0], dtype=np.int64)
                for _ in range(8):  # paging enumerates every hit: at most 36 on the stack, far fewer on mixed
                    page = _multi(sc, batch, 8, precision=prec, after=cur, d_r=d_r)
                    done = page["prim"][:, -1] < 0  # the list was not full: nothing follows its last hit
                    total += (page["prim"] >= 0).sum(1)
                    cur = M.next_cursors(page, cur)
                    more = _multi(sc, batch, 2, precision=prec, after=cur, d_r=d_r)
                    assert (more["prim"][done] == -1).all() and np.isinf(more["t"][done]).all()
                    if done.all():
                        break
                assert done.all() and total.sum() > batch.shape[0]
                if name == "stack" and family == "through":
                    assert total.max() > 8 * 3
        if name == "stack" and family == "through":
            straddle = (one["t"][:, 3] == one["t"][:, 4]) & (one["prim"][:, 4] >= 0)
            assert straddle.mean() > 0.05  # a tie across the boundary of pages of 2 (and of 1)
    sc.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", ["soup", "cornell"])
def test_first_slot_is_a_closest_hit(gpu, name):
    """k = 1 against the CPU oracle's closest hit, through the closest-hit certifier, on the batches of
    test_gpu_hit_edges.py (its soup: 150,000 triangles, the fp32 kernels' shallower collapse)."""
    from tests.test_gpu_hit_edges import batches as edge_batches
    data, families = edge_batches(name)
    sc = api.Scene(data).upload(gpu)
    for family, rays, want in families:
        d_r = _dev(rays)
        for prec, u, pname in PRECISIONS:
            got = _multi(sc, rays, 1, precision=prec, d_r=d_r)[:, 0]
            v = H.certify(rays, want, got, data.vertices, u)
            print(f"{name} {family} {pname}: {rays.shape[0]} rays, {v.summary()}")
            assert v.unexplained.size == 0, (name, family, pname, v.unexplained[:6].tolist())
            assert v.ratio < 1.0
    sc.close()


# ------------------------------------------------------------------------------------------------ 6
def test_padded_records(gpu, dev_lib, monkeypatch):
    """The PAD instantiations (one record per cache line: 128 bytes in fp64, 64 in fp32)."""
    monkeypatch.setenv("PRT_TUNE_TRI_STRIDE", "128")
    sc = api.Scene(M.scene("mixed")).upload(gpu)
    assert sc.bvh_info()["tri_stride"] == 128
    check_case(sc, "mixed", where=" padded")
    sc.close()


# ------------------------------------------------------------------------------------------------ 7
def test_lists_follow_a_refit(gpu):
    import torch
    data = M.scene("stack")
    _, rays, _ = M.batches("stack")[0]
    v = np.asarray(data.vertices, dtype=np.float64)
    v2 = v.copy()
    v2[..., 2] = v[..., 2] * 0.8 + 0.05 * np.sin(3.0 * v[..., 0]) + 0.1  # every layer bends and moves; the copies stay copies
    sc = api.Scene(data).upload(gpu)
    before = _multi(sc, rays, 8)
    d_v = torch.from_numpy(v2).cuda()
    sc.refit_device(d_v.data_ptr())
    for prec, u, pname in PRECISIONS:
        cert = M.Certifier(v2, rays, u)
        for k in (3, 8):
            got = _multi(sc, rays, k, precision=prec)
            s = cert.certify(rays, got)
            print(f"stack refitted {pname} k={k}: {s.summary()}")
            assert s.unexplained.size == 0 and s.entries > 0
    assert (_multi(sc, rays, 8)["t"] != before["t"]).mean() > 0.5
    sc.close()


# ------------------------------------------------------------------------------------------------ 8
def test_edges_and_errors(gpu):
    import torch
    data = M.scene("mixed")
    (_, edge, _), (_, axis, _) = M.batches("mixed")[:2]
    sc = api.Scene(data).upload(gpu)
    # n == 0, and the host call
    assert _multi(sc, edge[:0], 1).shape == (0, 1)
    assert sc.trace_multi(edge[:0], 1).shape == (0, 1)
    few = sc.trace_multi(edge[:777], 5, count_work=True)
    c = sc.counters()
    assert c["rays_closest"] == 777 and c["rays_shadow"] == 0 and c["samples"] == 0 and c["node_fetches"] > 0 and c["tri_tests"] > 0
    assert np.array_equal(_bytes(few), _bytes(_multi(sc, edge[:777], 5)))
    cur = M.next_cursors(few[:, :2])
    assert np.array_equal(_bytes(sc.trace_multi(edge[:777], 3, after=cur)), _bytes(few[:, 2:]))
    # exactly n * k records are written
    for prec, _, _ in PRECISIONS:
        for sort in (False, True):
            lists, behind = _multi(sc, edge[:1001], 3, precision=prec, sort=sort, guard=64)
            assert (behind == FILL).all() and not (lists["t"] == FILL).any()
            c = sc.counters()
            assert c["rays_closest"] == 1001 and c["rays_shadow"] == 0 and c["samples"] == 0 and c["kernel_ms"] > 0
    # refusals
    d_r = _dev(edge[:64])
    d_h = torch.zeros((64 * 8 + 1, 4), dtype=torch.float64, device="cuda")
    for kw, word in ((dict(k=0), "k must be"), (dict(k=9), "k must be"), (dict(k=2, off=8), "32-byte aligned"), (dict(k=2, precision=7), "precision")):
        for sort in (False, True):
            with pytest.raises(api.PrtError) as e:
                sc.trace_multi_device(d_r.data_ptr(), 64, kw["k"], d_h.data_ptr() + kw.get("off", 0), precision=kw.get("precision", 0), sort=sort)
            assert e.value.code == _abi.PRT_E_INVALID and word in str(e.value) and "prt_trace_multi" in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.trace_multi_device(None, 64, 2, d_h.data_ptr())
    assert e.value.code == _abi.PRT_E_INVALID
    # a NaN cursor on the device: no candidate after it
    cur = M.cursors(64)
    cur["t"][5] = np.nan
    got = _multi(sc, edge[:64], 2, after=cur)
    assert (got["prim"][5] == -1).all() and np.array_equal(_bytes(np.delete(got, 5, 0)), _bytes(np.delete(_multi(sc, edge[:64], 2), 5, 0)))
    # two calls in flight on two streams
    want = [_bytes(_multi(sc, r, 4)) for r in (edge, axis)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    h1, keep1 = _multi(sc, edge, 4, stream=s1.cuda_stream, sync=False)
    h2, keep2 = _multi(sc, axis, 4, stream=s2.cuda_stream, sync=False)
    torch.cuda.synchronize()
    for h, w, r in ((h1, want[0], edge), (h2, want[1], axis)):
        got = h.cpu().numpy()[:r.shape[0] * 4].view(_abi.HIT_DTYPE).reshape(r.shape[0], 4)
        assert np.array_equal(_bytes(got), w)
    sc.close()


# ------------------------------------------------------------------------------------------------ 9
def test_cpp_hits_equal_trace_multi(gpu, tmp_path):
    """Hittable::Hits (one ray, and the batch overload) on main.cpp's world equals Scene.trace_multi on the same rays."""
    build.build_host_example()
    exe = str(tmp_path / "hits_check")
    lib_dir = os.path.dirname(build.HOST_LIB)
    root = os.path.dirname(lib_dir)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "hits_check.cpp"), "-L", lib_dir,
                           "-Wl,-rpath," + lib_dir, "-lpooraytracer_host", "-lprt_hip", "-o", exe])
    data = scenes.cornell_box(ball_subdiv=2, width=48, height=40)
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    r = subprocess.run([exe, res, data.name, "300", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines() if line and line[0] != "#"])
    assert rows.shape == (300, 6 + 2 + 1 + 5)  # o, d, the domain, the number of records, their times
    rays = np.zeros(300, dtype=_abi.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmin"], rays["tmax"] = rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7]
    sc = api.Scene(data).upload(gpu)
    want = sc.trace_multi(rays, 5)
    sc.close()
    assert np.array_equal(rows[:, 8].astype(int), (want["prim"] >= 0).sum(1))
    assert np.array_equal(rows[:, 9:], np.where(want["prim"] >= 0, want["t"], -1.0))
    assert 0.3 * 300 < (rows[:, 8] >= 2).sum()
    assert "single-ray mismatches 0" in r.stdout
