"""CPU checks of the references in tests/device_math_model.py (against each other and against the oracle), of the case
counts of the box-test cases, of the gfx950 cross-build of the probe library, and of the product libraries' exports."""
import os
import subprocess

import mpmath
import numpy as np
import pytest

import oracle
from tests import device_math_model as M
from tests import test_slab_cpu as slab

mpf = mpmath.mpf
LD = np.longdouble


def test_longdouble_has_a_64_bit_mantissa_and_agrees_with_mpmath():
    assert np.finfo(LD).nmant >= 63
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.random(200), 2.0 ** rng.uniform(-1000, 1000, 200)])
    for name, f_ld, f_mp in (("sqrt", np.sqrt, mpmath.sqrt), ("rcp", lambda v: 1 / v, lambda v: 1 / v),
                             ("rsqrt", lambda v: 1 / np.sqrt(v), lambda v: 1 / mpmath.sqrt(v))):
        got = f_ld(x.astype(LD))
        for xi, gi in zip(x, got):
            ref = f_mp(mpf(float(xi)))
            rel = abs(M.mp_of(gi) - ref) / ref
            assert rel < mpf(2) ** -61, (name, xi, float(rel))
    # sin / cos over +-pi (sincos_turns' reference reduces by whole turns only) and beyond, to 2 pi (sincos_any's)
    a = np.concatenate([rng.uniform(-np.pi / 4, np.pi / 4, 200), rng.uniform(-np.pi, np.pi, 400), rng.uniform(0, 2 * np.pi, 200),
                        [np.pi, -np.pi, np.pi / 2, 2 * np.pi * (1 - 2.0 ** -31)]])
    for ai, si, ci in zip(a, np.sin(a.astype(LD)), np.cos(a.astype(LD))):
        assert abs(M.mp_of(si) - mpmath.sin(mpf(float(ai)))) < mpf(2) ** -62, ai
        assert abs(M.mp_of(ci) - mpmath.cos(mpf(float(ai)))) < mpf(2) ** -62, ai
    # pow_pos' reference exp(y log x) at |y log x| <= 50, on lattice x and the exponents the GPU test uses
    xs = np.concatenate([rng.integers(1, 1 << 31, size=150) / 2.0 ** 31, [2.0 ** -31, 1 - 2.0 ** -31, 0.5, np.nextafter(1.0, 0.0)]])
    for xi in xs:
        for yi in (1 / 2001.0, 1 / 41.0, 0.5, 1.0, 5.0, 40.0, 400.0, 2000.0):
            t = mpf(float(yi)) * mpmath.log(mpf(float(xi)))
            if abs(t) <= 50:
                got = np.exp(LD(yi) * np.log(LD(xi)))
                assert abs(M.mp_of(got) - mpmath.exp(t)) / mpmath.exp(t) < mpf(2) ** -56, (xi, yi)  # |t| 2^-63 relative at most


def test_longdouble_concentric_map_agrees_with_mpmath_including_both_sides_of_the_diagonals():
    rng = np.random.default_rng(4)
    k = rng.integers(0, 1 << 31, size=(300, 2))
    k[:20, 0] = 1 << 30                 # an axis
    k[20:40, 1] = 1 << 30
    k[40:60, 1] = k[40:60, 0]           # a diagonal
    k[60:80, 1] = (1 << 31) - k[60:80, 0]
    k[80] = (1 << 30, 1 << 30)
    u = k / 2.0 ** 31
    x, y = M.disk_concentric_ld(u[:, 0], u[:, 1])
    for i in range(u.shape[0]):
        rx, ry = M.disk_concentric_mp(u[i, 0], u[i, 1])
        assert abs(M.mp_of(x[i]) - rx) < mpf(2) ** -60 and abs(M.mp_of(y[i]) - ry) < mpf(2) ** -60, (k[i],)
        if 40 <= i < 80 and k[i, 0] != 1 << 30:  # continuous across |off.x| == |off.y|: either branch is the reference
            ax_, ay_ = M.disk_concentric_mp(u[i, 0], u[i, 1], force_first=True)
            bx_, by_ = M.disk_concentric_mp(u[i, 0], u[i, 1], force_first=False)
            assert abs(ax_ - bx_) < mpf(10) ** -50 and abs(ay_ - by_) < mpf(10) ** -50
    assert x[80] == 0 and y[80] == 0


def test_material_parameters_are_read_from_the_sources():
    """NS_VALUES and ETA_K of the GPU tests come from scenes.py and tests/*.py; the reader must find what is there."""
    from pooraytracer_amd import _abi, scenes
    ns, ek = M.ns_values_in_sources(), M.eta_k_in_sources()
    assert {0.5, 1.0, 5.0, 12.0, 20.0, 25.0, 40.0, 50.0, 60.0, 80.0, 400.0, 900.0, 2000.0} <= set(ns)
    assert {(0.1, 4.0), (0.5, 0.02), (1.5, 0.3), (0.2, 3.9), (0.9, 2.4), (1.1, 2.2), (1.5, 0.0), (1.33, 0.0), (2.4, 0.0)} <= set(ek)
    for data in (scenes.tiny_scene(), scenes.mixed_materials()):  # ... and what the scenes actually build
        for m in data.materials:
            if m.type == _abi.MAT_PHONG:
                assert float(m.ns) in ns, m.name
            if m.type == _abi.MAT_COOKTORRANCE:
                assert set(zip(map(float, m.eta), map(float, m.k))) <= set(ek), m.name


def test_alpha_values_are_read_from_the_sources():
    """The alpha pairs of the BSDF probes come from scenes.py and tests/*.py; the reader must find what is there."""
    from pooraytracer_amd import _abi, scenes
    al = M.alpha_values_in_sources()
    assert {(0.3, 0.3), (0.5, 0.5), (0.2, 0.6), (0.08, 0.5)} <= set(al)
    for data in (scenes.tiny_scene(), scenes.mixed_materials()):
        for m in data.materials:
            if m.type == _abi.MAT_COOKTORRANCE:
                assert (float(m.alpha_x), float(m.alpha_y)) in al, m.name
    assert {(1e-3, 1e-3), (1.0, 1.0), (0.01, 1.0)} <= set(M.bsdf_alphas()) and set(al) <= set(M.bsdf_alphas())
    mats = M.bsdf_materials()
    assert {tuple(r[14:16]) for r in mats["ct"]} == set(M.bsdf_alphas())
    assert {r[7] for r in mats["phong"]} == set(M.ns_values_in_sources()) and {r[16] for r in mats["phong"]} == {-1.0, 0.0, 1.0}
    assert {(e, k) for r in mats["ct"] for e, k in zip(r[8:11], r[11:14])} == set(M.eta_k_in_sources())
    assert all(np.float32(ns) == ns for ns in M.ns_values_in_sources())  # so inv_ns1 / spec_scale derive from the same ns in fp32


def test_fraction_fma_is_correctly_rounded_and_sees_what_an_unfused_pair_loses():
    # a * b = 1 + 2^-29 + 2^-60 exactly: rounding the product first drops 2^-60, which c = -1 then exposes
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0
    assert M.fma_exact(a, b, c) == 2.0 ** -29 + 2.0 ** -60
    assert a * b + c == 2.0 ** -29 and M.unfused_differs(a, b, c)
    assert M.fma_exact(3.0, 5.0, 7.0) == 22.0 and not M.unfused_differs(3.0, 5.0, 7.0)
    # the integer-ratio shortcut the GPU test uses on 10^5 operands is the Fraction result
    rng = np.random.default_rng(5)
    x, y = rng.uniform(-2, 2, 2000), rng.uniform(-2, 2, 2000)
    z = -x * y * (1 + rng.uniform(-1e-6, 1e-6, 2000))
    assert np.array_equal(M.fma_exact_many(x, y, z), np.array([M.fma_exact(p, q, r) for p, q, r in zip(x, y, z)]))
    f = np.float32
    assert M.fma_exact32(f(1 + 2.0 ** -12), f(1 + 2.0 ** -12), f(-1.0)) == f(2.0 ** -11 + 2.0 ** -24)
    # a tie: 1 + 2^-24 rounds to even (1.0)
    assert M.round_fraction_f32(M.Fraction(1) + M.Fraction(1, 1 << 24)) == f(1.0)
    assert M.round_fraction_f32(M.Fraction(1) + M.Fraction(3, 1 << 24)) == f(1 + 2.0 ** -22)


def test_rng_model_reproduces_the_oracle_stream_on_real_seeds():
    # the forward model on the oracle's own states: seed_keyed's hash restated
    def mix64(z):
        z &= (1 << 64) - 1
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & ((1 << 64) - 1)
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & ((1 << 64) - 1)
        return z ^ (z >> 31)
    for seed, pixel, sample in ((1, 0, 0), (7, 12345, 3), (2 ** 40 + 5, 64 * 64 - 1, 1023), (0, 1, 1)):
        key = mix64(seed + 0x9E3779B97F4A7C15)
        s = mix64(((((key >> 32) ^ (pixel + 1)) & 0xFFFFFFFF) << 32) | ((key ^ (sample + 1)) & 0xFFFFFFFF)) or 0x9E3779B97F4A7C15
        got, _ = M.rng_draws(np.array([s], dtype=np.uint64), 64)
        assert np.array_equal(got[0], oracle.rng_stream(seed, pixel, sample, 64)), (seed, pixel, sample)


def test_crafted_states_reproduce_any_pair_of_draws():
    rng = np.random.default_rng(9)
    k = rng.integers(0, 1 << 31, size=(100000, 2)).astype(np.uint64)
    k[:8] = [(0, 0), (0, (1 << 31) - 1), ((1 << 31) - 1, 0), (1 << 30, 1 << 30), (1, 1), ((1 << 31) - 1, (1 << 31) - 1), (0, 1 << 30), (1 << 30, 0)]
    got, _ = M.rng_draws(M.craft_state(k[:, 0], k[:, 1]), 2)
    assert np.array_equal(got, k.astype(np.float64) / 2.0 ** 31)
    k24 = rng.integers(0, 1 << 24, size=(100000, 2)).astype(np.uint64)
    got, _ = M.rng_draws(M.craft_state(k24[:, 0], k24[:, 1], shift=8), 2, f32=True)
    assert np.array_equal(got, k24.astype(np.float64) / 2.0 ** 24)


def test_visible_normal_restatement_is_a_unit_vector_on_the_upper_hemisphere_in_both_bases():
    for force in (True, False, None):
        for w in ((0.3, 0.1, 0.9), (0.3, 0.1, -0.9), (0.99, 0.0, 1e-3)):
            wm, info = M.ct_sample_wm_mp(0.2, 0.6, w, (0.7, 0.3), force_basis=force)
            assert abs(sum(c * c for c in wm) - 1) < mpf(10) ** -55 and wm[2] > 0
    # the switch: wh.z < 0.99999 takes the cross-product basis, normal incidence the fixed one
    _, info = M.ct_sample_wm_mp(0.5, 0.5, (0.0, 0.0, 1.0), (0.5, 0.5))
    assert not info["basis"] and info["whz"] == 1.0
    _, info = M.ct_sample_wm_mp(0.5, 0.5, (0.3, 0.1, 0.9), (0.5, 0.5))
    assert info["basis"] and abs(info["sin_h"] ** 2 + info["whz"] ** 2 - 1) < 1e-15
    # with the disk sample on the T1 axis and wh = z the warp leaves p alone: wm = normalize(ax px, 0 + ..., pz)
    wm, _ = M.ct_sample_wm_mp(1.0, 1.0, (0.0, 0.0, 1.0), (0.25, 0.0))
    assert abs(wm[0] - mpf(0.5)) < mpf(10) ** -55 and abs(wm[1]) < mpf(10) ** -55


def test_box_cases_hold_enough_accepted_and_enough_clearly_rejected_pairs():
    c = M.box_cases()
    n = c["o"].shape[0]
    assert (1 << 19) <= n <= (1 << 21)
    acc, rej = M.box_expectations(c)
    print(f"box cases: {n} pairs, exact accepts {int(acc.sum())}, clearly rejected {int(rej.sum())}")
    assert acc.sum() >= 10 ** 4 and rej.sum() >= 10 ** 4 and not (acc & rej).any()
    # the model's interval is exact_test's wherever tmax does not cut it
    sub = slice(0, n, 7)
    t0, t1 = M.exact_interval(c["o"][sub], c["d"][sub], c["lo"][sub], c["hi"][sub])
    with np.errstate(over="ignore"):  # 1 / d for the subnormal direction components among the cases
        assert np.array_equal(t1 > t0, slab.exact_test(c["o"][sub], c["d"][sub], c["lo"][sub], c["hi"][sub]))
    # the numpy emulation, both pad expressions: conservative on these cases, and rejecting the clear ones
    for variant in slab.PAD_VARIANTS:
        for s in range(0, n, 1 << 16):
            sl = slice(s, s + (1 << 16))
            g = c["grid"][s]
            with np.errstate(all="ignore"):
                got = slab.box_test(c["o"][sl], c["d"][sl], c["lo_q"][sl], c["hi_q"][sl], g[0], g[1:4], g[4:7],
                                    tmax=c["tmax"][sl].astype(np.float32), variant=variant)
            assert not (acc[sl] & ~got).any(), (variant, s)
            assert not (rej[sl] & got).any(), (variant, s)


def test_probe_cross_builds_for_gfx950_with_every_launcher():
    from pooraytracer_amd import build
    lib = build.build_probe()
    assert os.path.dirname(lib) == os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    missing = [s for s in M.probe_symbols() if s not in have]
    assert not missing, missing
    blob = open(lib, "rb").read()
    assert b"gfx950" in blob  # the device code object is in there
    M.probe_lib()  # loads without a GPU, every symbol resolves


def test_product_libraries_export_no_probe_symbol(prt_lib):
    from pooraytracer_amd import build
    for lib in (build.LIB, build.DEV_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        assert out.strip() and "prtprobe" not in out, lib


# ================================================================== the BSDF layer: model, bound, restatement, mutations
BSDF_CASES = [(n, p) for n in M.BSDF_OPS for p in ("f64", "f32")]


def test_bsdf_model_agrees_with_the_oracle_on_the_ordinary_strata():
    """The mpmath model of mat_eval / mat_scatter (fp64) against the ORACLE's Material::Eval / Scatter — code this work did
    not write — on random directions and the same seeded streams, to the suite's geometry tolerance of 1e-12 relative
    (per vector, against its largest component)."""
    from tests import test_materials as tm
    orc = oracle.Oracle(tm.DATA)
    dirs = M.direction_strata("f64")["random"]
    n = len(dirs)
    seed = 7
    states = np.array([M.seed_state(seed, i, 0) for i in range(n)], dtype=np.uint64)
    worst = 0.0
    for idx in (tm.M_LAMBERT, tm.M_PHONG50, tm.M_PHONG5, tm.M_MIRROR, tm.M_CT_ISO, tm.M_CT_ANISO, tm.M_GLASSY):
        raw = np.broadcast_to(np.array(M.raw_material(tm.DATA.materials[idx])), (n, M.MAT_NI))
        if idx != tm.M_MIRROR:  # (the mirror's Eval is not part of the layer: mat_eval returns 0 for it)
            wi, wo = dirs, dirs[::-1]
            R = M.bsdf_reference("mat_eval", "f64", np.concatenate([raw, wi, wo], 1), states)
            want = orc.material_eval(idx, wi, wo, seed=seed)
            got = R["ref"].astype(np.float64)
            ok = ~R["undef"] & ~R["knife"]
            rel = np.abs(got - want).max(1) / np.maximum(np.abs(want).max(1), 1e-300)
            rel[(np.abs(want).max(1) == 0) & (np.abs(got).max(1) == 0)] = 0
            assert ok.sum() >= 0.99 * n and rel[ok].max() <= 1e-12, (tm.DATA.materials[idx].name, "eval", float(rel[ok].max()))
            worst = max(worst, float(rel[ok].max()))
        rd = -dirs * np.array([1.0, -1.0, 1.0])  # wo = dirs in the frame n = z, t = x (bitangent = -y)
        frame = np.broadcast_to(np.array([0, 0, 1.0, 1.0, 0, 0]), (n, 6))
        R = M.bsdf_reference("mat_scatter", "f64", np.concatenate([raw, rd, frame], 1), states)
        wi_w, att, good = orc.material_scatter(idx, rd, seed=seed)
        ok = ~R["undef"] & ~R["knife"]
        assert ok.sum() >= 0.99 * n
        ref = R["ref"].astype(np.float64)
        assert np.array_equal(ref[ok, 0] == 1, good[ok]), tm.DATA.materials[idx].name
        both = ok & good
        lit = both & (np.abs(att).max(1) > 0) & np.isfinite(att).all(1)  # (below the horizon the reference leaves att unassigned)
        e_dir = np.abs(ref[both, 1:4] - wi_w[both]).max()
        e_att = (np.abs(ref[lit, 4:7] - att[lit]).max(1) / np.abs(att[lit]).max(1)).max()
        print(f"[bsdf] model vs oracle, {tm.DATA.materials[idx].name}: direction {e_dir:.3g}, att {e_att:.3g} relative ({int(both.sum())} samples)")
        assert e_dir <= 1e-12 and e_att <= 1e-12, (tm.DATA.materials[idx].name, e_dir, e_att)
        worst = max(worst, e_dir, e_att)
    print(f"[bsdf] model vs oracle: worst {worst:.3g}")


@pytest.mark.parametrize("name,prec", BSDF_CASES)
def test_bsdf_numpy_restatement_stays_inside_the_tolerance(name, prec):
    """The header's expressions in numpy, IEEE operations of the precision only, on every stratum of the GPU test: inside
    twice the running bound (the bound is not too tight), NaN-free wherever the exact value is finite, and the knife-edge
    inputs stay below 0.1 % of every stratum that is not knife-edge by construction (M.UNCAPPED_STRATA)."""
    R = M.bsdf_reference(name, prec)
    assert len(R["rows"]) <= 1 << 16
    got, after = M.bsdf_numpy(name, prec)
    ratio, fails = M.bsdf_compare(R, got, after if R["states"] is not None else None, what="numpy")
    assert not fails, fails
    # rows whose bound is infinite are held to finiteness and sign only: outside the grazing strata (the overflow window of
    # ct_D is what those are for) and the rim, they stay a small share of every stratum
    for st, sh in M.unbounded_share(R).items():
        assert st.startswith("grazing") or st in M.UNCAPPED_STRATA or sh <= 0.1, (st, sh)
    share = M.knife_edge_share(R)
    print(f"[bsdf] {name} {prec}: largest knife-edge share of a capped stratum {share:.4g}; undefined rows {int(R['undef'].sum())}")
    assert share <= 1e-3, share
    # undefined in exact arithmetic (nothing asserted): only ct_Dv at w.z == 0 with w . wm == 0, G1 / 0 * 0 — `wo.z == 0` returns
    # before any caller gets there
    assert R["undef"].sum() <= (1 if name == "ct_Dv" else 0), R["knife_names"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bsdf_strata_hold_every_material_class_and_what_their_names_say(prec):
    """Every stratum of the two material probes holds every material class it applies to (CookTorrance, Phong, Lambertian;
    for Scatter the mirror too), and the off-unit directions really have |w|^2 one and two ulp off 1 on either side."""
    want = {"mat_eval": {"random": {0, 1, 3}, "near_normal": {0, 1, 3}, "off_unit": {0, 1, 3}, "axes": {0, 1, 3},
                         "opposite_or_zero": {1, 3}, "grazing_one": {3}, "grazing_both": {3}, "rng_ends": {1}},
            "mat_scatter": {"random": {0, 1, 2, 3}, "random_tilted_frame": {0, 1, 2, 3}, "near_normal": {0, 1, 2, 3},
                            "off_unit": {0, 1, 2, 3}, "axes": {0, 1, 2, 3}, "grazing": {0, 1, 2, 3}, "zero": {0, 1, 3},
                            "rng_ends": {0, 1, 3}, "rng_rim": {0, 1}}}
    for name, strata in want.items():
        rows, states, strat = M.bsdf_inputs(name, prec)
        assert set(strat.tolist()) == set(strata), (name, sorted(set(strat.tolist())))
        for st, types in strata.items():
            have = {int(t): int(((strat == st) & (rows[:, 0] == t)).sum()) for t in types}
            assert all(c > 0 for c in have.values()) and set(rows[strat == st, 0].astype(int).tolist()) == types, (name, st, have)
        z = rows[:, 19] if name == "mat_eval" else -rows[:, 19]  # wi.z of Eval; wo.z of Scatter in the upright frame
        ct = rows[:, 0] == 3
        # CookTorrance meets the normal itself, the steps next to it and the axes
        nn = ct & (strat == "near_normal")
        step = 2.0 ** -23
        assert (z[nn] == 1).any() and ((z[nn] < 1) & (z[nn] >= 1 - 4 * step)).any(), name
        ax = ct & (strat == "axes")
        xy = rows[ax][:, 17:19]
        assert (xy[:, 0] == 0).any() and (xy[:, 1] == 0).any() and (np.abs(z[ax]) == 1).any(), name
    off = M.direction_strata(prec)["off_unit"]
    res = np.array([M.off_unit_residual(w, prec) for w in off])
    print(f"[bsdf] off_unit {prec}: |w|^2 - 1 in ulps of 1: {np.round(res, 2).tolist()}")
    assert np.abs(res - np.tile([-2, -1, 1, 2], 8)).max() <= 0.25
    assert np.array_equal(off, off.astype(M.PRECS[prec].dtype).astype(np.float64))


MUTATIONS = [("alpha_x for both axes", "ct_D"), ("alpha_x for both axes", "ct_lambda"), ("(1 + e) not squared", "ct_D"),
             ("ct_G = G1 * G1", "ct_G")]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mut,name", MUTATIONS)
def test_bsdf_tolerance_rejects_three_mutations(mut, name, prec):
    """The bound can fail: each mutation of the restatement leaves the tolerance on at least half of the ordinary stratum
    (random directions; anisotropic alphas, or the first mutation would be the identity)."""
    d = M.direction_strata(prec)["random"]
    al = np.array([(0.2, 0.6), (0.08, 0.5), (0.01, 1.0)])[np.arange(len(d)) % 3]
    rows = np.concatenate([al, d] + ([d[::-1]] if name == "ct_G" else []), 1)
    R = M.bsdf_reference(name, prec, rows)
    clean, _ = M.bsdf_numpy(name, prec, rows=R["rows"])
    bad, _ = M.bsdf_numpy(name, prec, mut=mut, rows=R["rows"])
    r0, f0 = M.bsdf_compare(R, clean, what="numpy")
    r1, _ = M.bsdf_compare(R, bad, what=f"numpy, mutated: {mut}")
    assert not f0 and (r0 <= 1).all()
    assert (r1 > 1).mean() >= 0.5, (mut, name, float((r1 > 1).mean()))
