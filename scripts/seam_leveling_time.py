"""Row f5 (global seam leveling) at a BASELINE config, with labels from the library's own view selection:
   seam_leveling_time.py --config 3 [--runs 3] [--out profiles/gsl_c3.json] [--no-model]
Records the device time per phase (mvs_gsl_stats: median of the timed runs after one warm-up), the CG iterations and errors per
channel, x rows, A / Gamma rows, patches, and the single-thread time of the CPU model (tests/tools/seam_model.cpp) on the same
input together with a bit-for-bit comparison of every output."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "tools")]
import numpy as np  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--no-model", action="store_true")
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "gsl_c%d.json" % a.config)

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
c.set_views(s.cams, s.images)
c.data_costs(M.Settings())
labels, ms = c.view_selection(s.adj_ptr, s.adj)
print("scene + labels: %.1f s, %d faces, %d views, %d unseen" % (time.perf_counter() - t0, s.n_faces, s.n_views, int((labels == 0).sum())), flush=True)

c.global_seam_leveling(s.adj_ptr, s.adj, labels)             # warm-up: buffers, code objects
runs = []
for _ in range(a.runs):
    t = time.perf_counter()
    got, st = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
    st["wall_ms"] = 1e3 * (time.perf_counter() - t)
    runs.append(st)
sysg = c.gsl_system()
c.close()
phases = ("ms_rows", "ms_patches", "ms_system", "ms_solve", "ms_output", "ms_total", "wall_ms")
med = {k: float(np.median([r[k] for r in runs])) for k in phases}
last = runs[-1]
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "views": s.n_views,
       "verts": int(len(s.verts)), "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "unseen_faces": int((labels == 0).sum()),
       "runs": a.runs, "ms_median": med, "ms_runs": [{k: r[k] for k in phases} for r in runs],
       "iterations": last["iterations"], "error": [float(e) for e in last["error"]],
       **{k: last[k] for k in ("patches", "merged", "x_rows", "a_rows", "gamma_rows", "lhs_nnz_lower", "seam_edges", "samples")},
       "note": "device time per phase from events on the context's stream (rows = vertex->faces, vertex rows, rings; patches = components, "
               "boxes, merges; system = A rows, b sampler, Lhs, Rhs; solve = Jacobi-preconditioned CG, three channels at once; output = "
               "mean and per-corner values); wall_ms = host clock around the call incl. input upload and output download"}
print(json.dumps({k: res[k] for k in ("ms_median", "iterations", "x_rows", "a_rows", "patches", "merged")}), flush=True)
if not a.no_model:
    import seam_model as SM
    t = time.perf_counter()
    stm, want, wst = SM.run_scene(s, labels)
    res["model_single_thread_s"] = time.perf_counter() - t
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32).ravel()
    lp, lc, lv = SM.lower_csr(want["lhs_ptr"], want["lhs_col"], want["lhs_val"])
    res["model_equal"] = bool(stm == 0 and np.array_equal(got["x_ptr"], want["x_ptr"]) and np.array_equal(got["x_label"], want["x_label"])
                              and np.array_equal(sysg["lhs_ptr"], lp) and np.array_equal(sysg["lhs_col"], lc) and np.array_equal(bits(sysg["lhs_val"]), bits(lv))
                              and np.array_equal(bits(sysg["b"]), bits(want["b"])) and np.array_equal(bits(sysg["rhs"]), bits(want["rhs"]))
                              and np.array_equal(bits(sysg["x_raw"]), bits(want["x_raw"])) and np.array_equal(bits(got["x_adjust"]), bits(want["x_adjust"]))
                              and np.array_equal(bits(got["corner_adjust"]), bits(want["corner_adjust"])) and wst["iterations"] == last["iterations"]
                              and np.array_equal(bits(wst["error"]), bits(last["error"])))
    print("model: %.1f s single thread, equal: %s" % (res["model_single_thread_s"], res["model_equal"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
