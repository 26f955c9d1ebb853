"""Account for every fp32 disagreement with the oracle; writes one JSON object.

  python tools/f32_accounting.py [--out profiles/f32_accounting.json]

Runs what tests/test_gpu_hit_edges.py and tests/test_gpu_f32_samples.py assert, through the same functions, and records
the figures they print:
  hits     per scene x builder (and `mixed` with padded records from the dev-hooks library) x ray family x precision: the
           certifier's verdict on the kernel's closest hits against the oracle's — rays whose primitive differs, by kind
           (lost / farther / tie / nearer / phantom), the unexplained ones (must be 0), the worst margin / bound among the
           explained ones and the worst |dt| / bound among same-primitive hits;
  samples  per matrix scene and max_depth: the share of fp32 samples not within 1e-4 of the oracle's sample, for the scene
           and per material class, with the median and maximum relative difference of the close ones; `reference_moved` is
           the same table for the oracle against itself with the eye moved by 2^-18 (what the caps sit above).
A failed condition raises, as in the tests.  One process, a few seconds of GPU time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f32_accounting.json"))
    args = ap.parse_args()

    from pooraytracer_amd import api, build
    from tests import hit_certifier as H, sample_classes as S
    from tests import test_gpu_f32_samples as TS, test_gpu_hit_edges as TH
    build.build()
    if api.device_count() < 1:
        raise SystemExit("f32_accounting: no HIP device")

    def rows(report):
        return {f"{family}/{prec}": s for (family, prec), s in report.items()}

    hits = {}
    for name in sorted(TH.SCENES):
        for device_bvh in (False, True):
            sc = api.Scene(TH.batches(name)[0], device_bvh=device_bvh).upload(0)
            hits[f"{name}/{'device' if device_bvh else 'host'}-bvh"] = rows(TH.check_case(sc, name))
            sc.close()
    os.environ["PRT_TUNE_TRI_STRIDE"] = "128"
    with api.dev_hooks():
        sc = api.Scene(TH.batches("mixed")[0]).upload(0)
        assert sc.bvh_info()["tri_stride"] == 128
        hits["mixed/host-bvh/padded"] = rows(TH.check_case(sc, "mixed"))
        sc.close()
    del os.environ["PRT_TUNE_TRI_STRIDE"]

    samples, moved = {}, {}
    for perm, lighting in S.CASES:
        for depth in S.DEPTHS:
            key = f"{perm}/{lighting}/depth{depth}"
            rep = TS.class_report(perm, lighting, depth)
            S.show(key, rep)
            assert S.over_cap(rep, depth) == [], (key, S.over_cap(rep, depth))
            samples[key] = rep
            ref, trace = S.oracle_samples(perm, lighting, depth)
            shifted, _ = S.oracle_samples(perm, lighting, depth, shifted=True)
            moved[key] = S.shares(shifted, ref, S.classes(S.scene(perm, lighting), trace))

    fp32 = [(k, s) for case in hits.values() for k, s in case.items() if k.endswith("/f32")]
    disagree = [s["disagree"] / (TH.N_EDGE if k.startswith("edge") else TH.N_AXIS) for k, s in fp32]
    worst_class = max((r["not_close"], f"{key}:{name}") for key, rep in samples.items() for name, r in rep.items()
                      if name != "scene" and r["samples"] >= S.MIN_CLASS)
    out = {
        "what": "tools/f32_accounting.py: every fp32 (and fp64) disagreement with the oracle, certified; fp32 samples by class",
        "certifier": {"c": H.C_BOUND, "same_tol": {"f32": H.SAME_TOL[H.U32], "f64": H.SAME_TOL[H.U64]},
                      "rays": {"edge": TH.N_EDGE, "axis": TH.N_AXIS}},
        "summary": {
            "unexplained": sum(s["unexplained"] for case in hits.values() for s in case.values()),
            "fp32_worst_ratio": max(s["worst_ratio"] for _, s in fp32),
            "fp32_worst_same_prim_dt_ratio": max(s["same_prim_dt_ratio"] for _, s in fp32),
            "fp32_disagree_share_min_max": [min(disagree), max(disagree)],
            "worst_scene_not_close": {f"depth{d}": max(rep["scene"]["not_close"] for key, rep in samples.items()
                                                        if key.endswith(f"depth{d}")) for d in S.DEPTHS},
            "worst_class_not_close": {"share": worst_class[0], "where": worst_class[1]},
        },
        "caps": {"class": S.CAP_CLASS, "scene": {f"depth{d}": c for d, c in S.CAP_SCENE.items()}, "close_rel": S.CLOSE_REL,
                 "min_class_samples": S.MIN_CLASS},
        "hits": hits,
        "samples": samples,
        "reference_moved": moved,
    }
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"]))


if __name__ == "__main__":
    main()
