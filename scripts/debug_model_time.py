"""Row f10 (the view-selection debug model) at a BASELINE config, with labels from the library's own view selection:
   debug_model_time.py --config 3 [--runs 3] [--out profiles/debug_model_c3.json]
Records the device time (events on the context's stream; median of the timed runs after one warm-up) of debug_views_kernel -- the debug
images of all the config's views in one call, left on the device -- and of debug_patch_kernel (mvs_patch_stats.ms_resolve of
Context.debug_patches), the bytes each of them stores and the bandwidth that implies, and in the same run on the same device a plain
device-to-device copy of the same number of bytes.  Both kernels are pure store streams: they read a 144-entry table and a header per
image or patch."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "debug_model_c%d.json" % a.config)


def copy_gbs(nbytes, reps=5):
    """GB/s (read + write counted) of a device-to-device copy that moves nbytes in total: nbytes / 2 read, nbytes / 2 written"""
    n = max(int(nbytes) // 2, 1)
    src = torch.empty(n, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    src.zero_(); dst.copy_(src); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return 2 * n / (float(np.median(ms)) * 1e-3) / 1e9, float(np.median(ms))


def stream(nbytes, ms):
    gbs, cms = copy_gbs(nbytes)
    own = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else None
    return {"bytes": int(nbytes), "ms": ms, "gb_per_s": own, "device_copy_same_bytes_gb_per_s": gbs, "device_copy_same_bytes_ms": cms,
            "share_of_copy": own / gbs if own else None}


t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
c.set_views(s.cams, s.images)
c.data_costs(M.Settings())
labels, ms = c.view_selection(s.adj_ptr, s.adj)
print("scene + labels: %.1f s, %d faces, %d views, %d unseen" % (time.perf_counter() - t0, s.n_faces, s.n_views, int((labels == 0).sum())), flush=True)

# ---- debug_views_kernel: the debug images of all views, on the device ----
sizes = [(im.shape[1], im.shape[0]) for im in s.images]
view_bytes = 3 * sum(w * h for w, h in sizes)
buf = torch.empty(view_bytes, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
c.set_option("profile", 1)
c.debug_embeddings(sizes, out=buf); c.get_profile()                              # warm-up
views_ms = []
for _ in range(a.runs):
    c.debug_embeddings(sizes, out=buf)
    views_ms.append(c.get_profile()["debug_views"][0])
c.set_option("profile", 0)
sample = buf[:3 * sizes[0][0] * sizes[0][1]].cpu().numpy()
import debug_model as DM  # noqa: E402
views_ok = bool(np.array_equal(sample, DM.image(sizes[0][0], sizes[0][1], 0, 0).ravel()))
del buf

# ---- debug_patch_kernel ----
c.debug_patches(s.adj_ptr, s.adj, labels, on_device=True)                        # warm-up: buffers, code objects
runs = []
for _ in range(a.runs):
    t = time.perf_counter()
    got, st = c.debug_patches(s.adj_ptr, s.adj, labels, on_device=True)
    st["wall_ms"] = 1e3 * (time.perf_counter() - t)
    runs.append(st)
phases = ("ms_tables", "ms_lists", "ms_resolve", "ms_total", "wall_ms")
med = {k: float(np.median([r[k] for r in runs])) for k in phases}
last = runs[-1]
NP = last["pixels"]
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "views": s.n_views,
       "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "unseen_faces": int((labels == 0).sum()), "runs": a.runs,
       **{k: last[k] for k in ("patches", "merged", "listed_faces", "pixels", "valid_pixels")},
       "debug_views_kernel": dict(stream(view_bytes, float(np.median(views_ms))), ms_runs=views_ms, first_image_equals_the_restatement=views_ok),
       "debug_patch_kernel": dict(stream(14 * NP, med["ms_resolve"]), ms_runs=[r["ms_resolve"] for r in runs]),
       "debug_patches_ms_median": med,
       "note": "bytes = what the kernel stores (views: 3 B per pixel; patches: 12 B image + 2 mask bytes per pixel); neither reads more than a "
               "144-entry table and one header per image / patch; the copy moves the same number of bytes, half read and half written"}
print(json.dumps({k: res[k] for k in ("pixels", "debug_views_kernel", "debug_patch_kernel", "debug_patches_ms_median")}), flush=True)
c.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
