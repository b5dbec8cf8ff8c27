"""Row f7 (local seam leveling) at a BASELINE config, with labels from the library's own view selection, the adjustments of its global
seam leveling and the patches of its row f6, which stay on the device:
   local_seam_leveling_time.py --config 3 [--runs 3] [--out profiles/lsl_c3.json] [--no-model]
Records the device time per phase (mvs_lsl_stats: median of the timed runs after one warm-up, device events), the counters, the solve's
iterations, the share of patches and pixels on the global-memory path, the LDS and HBM rates the solve reaches (bytes per
unknown and iteration counted from the kernel: 3 channels x (pass 1: 5 reads of p; pass 2: 5 reads of p, r read and written; pass 3: r
read, p read and written) = 204 B of LDS plus 3 x 4 B of the unknown list per pass, and 24 B of x in global memory) beside the
guide's ceilings (LDS ~75 TB/s for 4-byte reads with every CU streaming, HBM 6.3 TB/s), and the single-thread time of the CPU model
(tests/tools/blend_model.cpp) on the same input with a bit-for-bit comparison of all three output arrays and every counter."""
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
out_path = a.out or os.path.join(ROOT, "profiles", "lsl_c%d.json" % a.config)

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
c.set_views(s.cams, s.images)
c.data_costs(M.Settings())
labels, ms = c.view_selection(s.adj_ptr, s.adj)
gsl, gst = c.global_seam_leveling(s.adj_ptr, s.adj, labels)
dev, pst = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], on_device=True)
print("scene + labels + rows f5, f6: %.1f s, %d faces, %d views, %d patches, %d pixels" % (time.perf_counter() - t0, s.n_faces, s.n_views, pst["patches"], pst["pixels"]), flush=True)

c.local_seam_leveling(s.adj_ptr, s.adj, labels, dev, on_device=True)             # warm-up: buffers, code objects
runs = []
for _ in range(a.runs):
    t = time.perf_counter()
    got, st = c.local_seam_leveling(s.adj_ptr, s.adj, labels, dev, on_device=True)
    st["wall_ms"] = 1e3 * (time.perf_counter() - t)
    runs.append(st)
phases = ("ms_topology", "ms_colours", "ms_writes", "ms_mask", "ms_solve", "ms_total", "wall_ms")
med = {k: float(np.median([r[k] for r in runs])) for k in phases}
last = runs[-1]
solved = max(last["patches_lds"] + last["patches_global"], 1)
mean_iters = last["iterations_total"] / (3.0 * solved)
unknown_iterations = last["strip_pixels"] * mean_iters            # an estimate: patches weigh equally in mean_iters
lds_bytes = (204 + 36) * unknown_iterations
hbm_bytes = 24 * unknown_iterations
counters = [k for k in M.viewsel.LSL_COUNTS] + ["iterations_max"]
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "views": s.n_views,
       "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "patches": pst["patches"], "pixels": pst["pixels"],
       "valid_pixels": pst["valid_pixels"], "params": {k: getattr(M.default_lsl_params(), k) for k in ("tolerance", "max_iterations", "strip_width", "lds_bytes")},
       "runs": a.runs, "ms_median": med, "ms_runs": [{k: r[k] for k in phases} for r in runs],
       **{k: last[k] for k in counters}, "error_max": last["error_max"],
       "strip_share_of_valid": last["strip_pixels"] / max(pst["valid_pixels"], 1),
       "global_path": {"patches_share": last["patches_global"] / solved, "pixels_share": last["pixels_global"] / max(pst["pixels"], 1)},
       "solve": {"mean_iterations": mean_iters, "unknown_iterations_estimate": unknown_iterations,
                 "lds_tb_per_s": lds_bytes / (med["ms_solve"] * 1e-3) / 1e12 if med["ms_solve"] > 0 else None, "lds_ceiling_tb_per_s": 75.0,
                 "global_tb_per_s": hbm_bytes / (med["ms_solve"] * 1e-3) / 1e12 if med["ms_solve"] > 0 else None, "hbm_ceiling_tb_per_s": 6.3},
       "note": "device time per phase from events on the context's stream (topology = keys, sort, infos, seam edges, edge projections; colours = "
               "edge and vertex samples; writes = clearing the winner words, copying image and mask, mark and write passes; mask = distance passes, "
               "prepared mask, unknowns, ranks; solve = all conjugate-gradient iterations of all patches, one launch per LDS tier); wall_ms = host "
               "clock around the call; inputs and outputs stay on the device"}
print(json.dumps({k: res[k] for k in ("ms_median", "strip_pixels", "iterations_max", "global_path", "solve")}), flush=True)

if not a.no_model:
    import blend_model as BM
    import torch

    def dev_host(d, dtype):
        dt = np.dtype(dtype); n = d.shape[0]
        if n == 0:
            return np.zeros(0, dt)

        class _Dev:
            __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (d.data_ptr(), False), "version": 2}
        return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt)
    host = {k: dev_host(got[k], dt) for k, dt in (("image", np.float32), ("validity", np.uint8), ("blending", np.uint8))}
    pa, _ = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"])
    BM.build()
    t = time.perf_counter()
    stm, want, wst, _ = BM.run_scene(s, labels, pa)
    res["model_single_thread_s"] = time.perf_counter() - t
    ok = stm == 0 and all(last[k] == wst[k] for k in BM.STATS)
    ok = ok and np.float32(last["error_max"]).view(np.uint32) == np.float32(wst["error_max"]).view(np.uint32)
    for k in ("image", "validity", "blending"):
        ok = ok and np.array_equal(host[k].view(np.uint8).ravel(), np.ascontiguousarray(want[k]).view(np.uint8).ravel())
    res["model_equal"] = bool(ok)
    print("model: %.1f s single thread, equal: %s" % (res["model_single_thread_s"], res["model_equal"]), flush=True)
c.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
