"""Accuracy of row f7's solve (CPU only: the model is bit-equal to the device).  For every case of tests/test_local_seam_model.py's
accuracy_cases() and every tolerance 1e-4 .. 1e-7: the largest |model - fp64 direct solve| over all unknowns and channels, the same
figure for an fp32 SuperLU solve of the same systems, the iterations.  The default tolerance is the loosest power of ten whose worst
value stays below half the ceiling (2^-12); the default max_iterations is four times the measured maximum at that tolerance, rounded up
to the next hundred.  Writes profiles/lsl_accuracy.json.

    python scripts/lsl_accuracy.py [--out profiles/lsl_accuracy.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")):
    sys.path.insert(0, p)


def main():
    import mvs_texturing_amd as M
    import blend_model as BM, patch_model as PM, seam_model as SM
    import test_local_seam_model as T
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lsl_accuracy.json")
    M.synth.build_synth(); SM.build(); PM.build(); BM.build()
    tolerances = [1e-4, 1e-5, 1e-6, 1e-7]
    cases = list(T.accuracy_cases())
    rows = []
    for name, g, labels, pa in cases:
        row = dict(case=name, patches=int(len(pa["label"])), pixels=int(len(pa["validity"])))
        for tol in tolerances:
            worst, worst32, unknowns, stats = T.measure_accuracy(g, labels, pa, tolerance=tol, max_iterations=100000)
            row["unknowns"] = unknowns; row["fp32_lu"] = worst32
            row["tol_%g" % tol] = dict(worst=worst, iterations_max=stats["iterations_max"], error_max=stats["error_max"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    half = 2.0 ** -12
    worst_at = {tol: max(r["tol_%g" % tol]["worst"] for r in rows) for tol in tolerances}
    chosen = next(tol for tol in tolerances if worst_at[tol] < half)
    it_max = max(r["tol_%g" % chosen]["iterations_max"] for r in rows)
    acc = dict(ceiling=2.0 ** -11, half_ceiling=half, tolerance=chosen, worst_model=worst_at[chosen],
               worst_by_tolerance={"%g" % t: worst_at[t] for t in tolerances}, worst_fp32_lu=max(r["fp32_lu"] for r in rows),
               iterations_max_measured=it_max, max_iterations=-(-4 * it_max // 100) * 100, cases=rows)
    with open(out_path, "w") as f:
        json.dump(acc, f, indent=1)
    print("tolerance %g: worst %.3e (half ceiling %.3e), iterations max %d -> max_iterations %d" % (chosen, acc["worst_model"], half, it_max, acc["max_iterations"]))


if __name__ == "__main__":
    main()
