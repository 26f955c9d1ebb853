"""CPU tests of the multi-hit queries (prt_trace_multi, include/prt.h): the numpy model is a fit reference under its own
list certifier, the certifier flags every planted fault, the batches are no empty test (lists longer than the capacity,
exact ties), the ABI is additive, and what can be said without a GPU (the wrapper's refusals, PRT_E_NO_DEVICE)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes
from tests import hit_certifier as H
from tests import multi_hit_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = _abi.MULTI_HIT_MAX


# ------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", sorted(M.SCENES))
def test_model_is_a_fit_reference(name):
    """On every scene and batch of the GPU tests, as generated and with the interval opened to the whole line: the float64
    lists are certified at u = 2^-53 (judged in long double), the float32 lists at u = 2^-24 (judged in float64)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here: nothing to judge the fp64 lists with")
    v = M.scene(name).vertices
    for family, rays, pr in M.batches(name):
        for u, dtype in ((H.U64, np.float64), (H.U32, np.float32)):
            cert = M.certifier(name, family, u)
            for which, batch in (("as generated", rays), ("whole line", M.whole_line(rays))):
                got, ncand = M.model_hits(v, batch, dtype, K, pr=pr)
                s = cert.certify(batch, got).summary()
                print(f"{name} {family} {np.dtype(dtype).name} {which}: {batch.shape[0]} rays, {ncand.mean():.2f} candidates per ray, {s}")
                assert s["unexplained"] == 0, (name, family, which, s)
                # no empty test: completeness is asserted on a fair share of what is listed (the batches AIM at edges, and
                # on the soup's small triangles in fp32 most of those hits are within their bound of one)
                assert s["entries"] > 0 and s["robust_candidates"] > 0.25 * s["entries"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_pages_are_the_one_call(dtype):
    """The model itself obeys the paging contract, also where a tie straddles a page: four pages of 2 = one call of 8."""
    v = M.scene("stack").vertices
    _, rays, pr = M.batches("stack")[0]
    one = M.model_hits(v, rays, dtype, 8, pr=pr)[0]
    cur, pages = None, []
    for _ in range(4):
        page = M.model_hits(v, rays, dtype, 2, after=cur, pr=pr)[0]
        pages.append(page)
        cur = M.next_cursors(page, cur)
    assert np.array_equal(np.concatenate(pages, 1).view(np.uint8), one.view(np.uint8))
    straddle = (one["t"][:, 3] == one["t"][:, 4]) & (one["prim"][:, 4] >= 0)
    assert straddle.mean() > 0.05
    assert (M.model_hits(v, rays, dtype, 2, after=M.next_cursors(M.model_hits(v, rays, dtype, 40, pr=pr)[0]), pr=pr)[0]["prim"] == -1).all()


# ------------------------------------------------------------------------------------------------- planted faults
def _stack_lists():
    v = M.scene("stack").vertices
    _, rays, pr = M.batches("stack")[0]
    got, ncand = M.model_hits(v, rays, np.float64, K, pr=pr)
    return rays, got, ncand, M.certifier("stack", "through", H.U64)


def _flagged(cert, rays, got, rows, reason, after=None):
    v = cert.certify(rays, got, after)
    assert reason in v.reasons, (reason, v.summary())
    assert np.isin(rows, v.unexplained).all(), (reason, v.summary())
    return v


def test_planted_faults_are_flagged():
    rays, got, ncand, cert = _stack_lists()
    assert cert.certify(rays, got).unexplained.size == 0
    full = np.flatnonzero((got["prim"][:, -1] >= 0) & (got["t"][:, 1] > got["t"][:, 0]) & (got["t"][:, 3] > got["t"][:, 2]))[:50]
    assert full.size == 50
    # a dropped hit in the middle of a list: the rest moves up, the last slot becomes a miss
    bad = got.copy()
    bad[full, 2:-1] = got[full, 3:]
    bad["t"][full, -1], bad["prim"][full, -1] = np.inf, -1
    bad["alpha"][full, -1] = bad["beta"][full, -1] = 0
    bad["front"][full, -1] = 0
    v = cert.certify(rays, bad)
    assert "lost_robust" in v.reasons and np.isin(full, v.unexplained).mean() > 0.9, v.summary()  # (a non-robust one may go)
    # two entries swapped
    bad = got.copy()
    bad[full, 0], bad[full, 1] = got[full, 1], got[full, 0]
    _flagged(cert, rays, bad, full, "not_ascending")
    # an exact tie reported in descending prim
    tie = np.flatnonzero((got["t"][:, 1:] == got["t"][:, :-1]).any(1) & (got["prim"][:, -1] >= 0))[:50]
    assert tie.size == 50
    bad = got.copy()
    for r in tie:
        j = int(np.argmax(got["t"][r, 1:] == got["t"][r, :-1]))
        bad[r, j], bad[r, j + 1] = got[r, j + 1], got[r, j]
    _flagged(cert, rays, bad, tie, "not_ascending")
    # a primitive reported twice
    bad = got.copy()
    bad[full, 1] = got[full, 0]
    _flagged(cert, rays, bad, full, "prim_twice")
    # a hit moved by 1e-3 of its distance (kept in order: the next one is a layer away)
    bad = got.copy()
    bad["t"][full, 0] = got["t"][full, 0] * (1 - 1e-3)
    _flagged(cert, rays, bad, full, "entry_no_hit")
    # the wrong face
    bad = got.copy()
    bad["front"][full, 2] = 1 - got["front"][full, 2]
    _flagged(cert, rays, bad, full, "front")
    # a candidate at the cursor, and one before it
    cur = M.next_cursors(got[:, :2])
    page = M.model_hits(M.scene("stack").vertices, rays, np.float64, 2, after=cur, pr=M.batches("stack")[0][2])[0]
    assert cert.certify(rays, page, cur).unexplained.size == 0
    for col in (1, 0):
        bad = page.copy()
        bad[full, 0] = got[full, col]
        _flagged(cert, rays, bad, full, "at_or_before_cursor", after=cur)


# ------------------------------------------------------------------------------------------------- no empty test
def test_the_batches_hold_long_lists_and_exact_ties():
    v = M.scene("stack").vertices
    _, rays, pr = M.batches("stack")[0]
    first9, ncand = M.model_hits(v, rays, np.float64, 9, pr=pr)
    long, ties = float((ncand > 8).mean()), M.tie_share(first9)
    print(f"stack through: {long:.3f} of the rays have more than 8 candidates, {ties:.3f} an exact tie among their first 9")
    assert long >= 0.90 and ties >= 0.05
    for name in ("cornell", "mixed"):
        for family, rays, pr in M.batches(name):
            ties = M.tie_share(M.model_hits(M.scene(name).vertices, rays, np.float64, K, pr=pr)[0])
            print(f"{name} {family}: {ties:.4f} of the rays have an exact tie among their first {K}")
            assert ties >= 0.01, (name, family, ties)


# ------------------------------------------------------------------------------------------------- ABI and wrapper
def test_abi_is_additive(prt_lib, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "prt.h"\nint main(){printf("%d %zu %d\\n",PRT_ABI_VERSION,sizeof(PrtHitCursor),'
                   "PRT_MULTI_HIT_MAX);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["6", "16", "8"]
    assert _abi.PRT_ABI_VERSION == 6 and prt_lib.prt_abi_version() == 6 and _abi.MULTI_HIT_MAX == 8
    assert C.sizeof(_abi.PrtHitCursor) == _abi.HIT_CURSOR_DTYPE.itemsize == 16
    for f, _ in _abi.PrtHitCursor._fields_:
        assert getattr(_abi.PrtHitCursor, f).offset == _abi.HIT_CURSOR_DTYPE.fields[f][1]
    for name in ("prt_trace_multi", "prt_trace_multi_device", "prt_trace_multi_sorted_device"):
        assert name in _abi.EXPORTS and hasattr(prt_lib, name)


def test_queries_fail_loudly_without_upload(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    rays = scenes.camera_rays(scenes.tiny_scene().camera, 5)
    with pytest.raises(api.PrtError) as e:
        sc.trace_multi(rays, 3)
    assert e.value.code == _abi.PRT_E_NO_DEVICE and "prt_trace_multi:" in str(e.value)
    for sort, who in ((False, "prt_trace_multi_device:"), (True, "prt_trace_multi_sorted_device:")):
        with pytest.raises(api.PrtError) as e:
            sc.trace_multi_device(256, 5, 3, 512, sort=sort)
        assert e.value.code == _abi.PRT_E_NO_DEVICE and who in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.trace_multi(rays[:0], 1)  # no ray, still no device
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    sc.close()


def test_host_call_refuses_a_bad_cursor_or_k(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    rays = scenes.camera_rays(scenes.tiny_scene().camera, 4)
    hits = np.zeros((4, 9), dtype=_abi.HIT_DTYPE)
    for k in (0, 9, -1):
        assert prt_lib.prt_trace_multi(sc._h, rays.ctypes.data, None, 4, k, hits.ctypes.data, 0) == _abi.PRT_E_INVALID
        assert "prt_trace_multi" in prt_lib.prt_last_error().decode()
    assert prt_lib.prt_trace_multi(sc._h, None, None, 4, 2, hits.ctypes.data, 0) == _abi.PRT_E_INVALID
    assert prt_lib.prt_trace_multi(sc._h, rays.ctypes.data, None, 4, 2, None, 0) == _abi.PRT_E_INVALID
    assert prt_lib.prt_trace_multi(None, rays.ctypes.data, None, 4, 2, hits.ctypes.data, 0) == _abi.PRT_E_INVALID
    cur = M.cursors(4)
    cur["t"][2] = np.nan
    with pytest.raises(api.PrtError) as e:
        sc.trace_multi(rays, 2, after=cur)
    assert e.value.code == _abi.PRT_E_INVALID and "cursor 2" in str(e.value) and "NaN" in str(e.value)
    cur = M.cursors(4)
    cur["reserved"][1] = 7
    with pytest.raises(api.PrtError) as e:
        sc.trace_multi(rays, 2, after=cur)
    assert e.value.code == _abi.PRT_E_INVALID and "cursor 1" in str(e.value) and "reserved" in str(e.value)
    with pytest.raises(api.PrtError) as e:  # legal cursors (the neutral one, +inf) get as far as the missing device
        cur = M.cursors(4)
        cur["t"][0] = np.inf
        sc.trace_multi(rays, 2, after=cur)
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    sc.close()


def test_wrapper_raises_shape_and_dtype_errors_before_any_call(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    rays = scenes.camera_rays(scenes.tiny_scene().camera, 4)
    with pytest.raises(TypeError):
        sc.trace_multi(rays.tolist(), 2)
    with pytest.raises(TypeError):
        sc.trace_multi(np.zeros((4, 8)), 2)
    with pytest.raises(ValueError):
        sc.trace_multi(rays.reshape(2, 2), 2)
    with pytest.raises(TypeError):
        sc.trace_multi(rays, 2.0)
    with pytest.raises(TypeError):
        sc.trace_multi(rays, True)
    for k in (0, 9):
        with pytest.raises(ValueError):
            sc.trace_multi(rays, k)
    with pytest.raises(TypeError):
        sc.trace_multi(rays, 2, after=np.zeros((4, 2)))
    with pytest.raises(TypeError):
        sc.trace_multi(rays, 2, after=[(0.0, -1, 0)] * 4)
    with pytest.raises(ValueError):
        sc.trace_multi(rays, 2, after=M.cursors(3))
    sc.close()
