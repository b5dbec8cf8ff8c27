"""Row f6 (texture patches + adjust_colors) at a BASELINE config, with labels from the library's own view selection and the
adjustments of its own global seam leveling:
   texture_patches_time.py --config 3 [--runs 3] [--out profiles/patches_c3.json] [--no-model] [--window 64] [--tone-mapping gamma]
Records pixels, the valid share, the device time per phase (mvs_patch_stats: median of the timed runs after one warm-up, device
events), the bytes the two streaming phases must move and the bandwidth that implies beside a plain device-to-device copy of the same
number of bytes on the same device (measured here with events), and the single-thread time of the CPU model
(tests/tools/patch_model.cpp) on the same input with a bit-for-bit comparison.  The outputs stay on the device (out_on_device); with
--window N the comparison reads back only the first, the largest and N evenly spaced patches instead of a host copy of everything.
--tone-mapping gamma runs rows f5 and f6 in that mode (the CPU model states `none` only: no comparison then; the default output becomes
profiles/patches_c<config>_gamma.json).  scripts/tone_mapping_time.py measures the two modes side by side."""
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
ap.add_argument("--no-model", action="store_true")
ap.add_argument("--window", type=int, default=0, help="compare this many patches (plus the first and the largest) instead of all")
ap.add_argument("--tone-mapping", default="none", choices=["none", "gamma"])
a = ap.parse_args()
TONE = M.viewsel.TONE_MAPPINGS[a.tone_mapping]
if TONE:
    a.no_model = True
out_path = a.out or os.path.join(ROOT, "profiles", "patches_c%d%s.json" % (a.config, "_gamma" if TONE else ""))


def dev_bytes(dev, nbytes, offset=0):
    """nbytes of a context-owned device array from byte `offset`, through torch"""
    if nbytes == 0:
        return np.zeros(0, np.uint8)

    class _Dev:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (dev.data_ptr() + offset, False), "version": 2}
    return torch.as_tensor(_Dev(), device="cuda").cpu().numpy()


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


t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
c.set_views(s.cams, s.images)
c.data_costs(M.Settings())
labels, ms = c.view_selection(s.adj_ptr, s.adj)
gsl, gst = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(tone_mapping=TONE))
ca = gsl["corner_adjust"]
print("scene + labels + seam leveling: %.1f s, %d faces, %d views, %d unseen" % (time.perf_counter() - t0, s.n_faces, s.n_views, int((labels == 0).sum())), flush=True)

# the size first, without allocating the pixel arrays
try:
    c.texture_patches(s.adj_ptr, s.adj, labels, ca, params=M.default_patch_params(max_pixels=1, tone_mapping=TONE), on_device=True)
    sized = None
except M.MvsError as e:
    sized = e.stats
print("size:", json.dumps({k: sized[k] for k in ("patches", "merged", "listed_faces", "pixels")} if sized else None), flush=True)

PP = M.default_patch_params(tone_mapping=TONE)
c.texture_patches(s.adj_ptr, s.adj, labels, ca, PP, on_device=True)         # warm-up: buffers, code objects
runs = []
for _ in range(a.runs):
    t = time.perf_counter()
    got, st = c.texture_patches(s.adj_ptr, s.adj, labels, ca, PP, on_device=True)
    st["wall_ms"] = 1e3 * (time.perf_counter() - t)
    runs.append(st)
phases = ("ms_tables", "ms_lists", "ms_mark", "ms_resolve", "ms_total", "wall_ms")
med = {k: float(np.median([r[k] for r in runs])) for k in phases}
last = runs[-1]
NP = last["pixels"]
# bytes the streaming phases cannot avoid: the mark phase clears the two winner words (8 B / pixel; its atomics come on top and are
# not counted); resolve reads them (8), reads the view's pixel (3) and writes the image (12) and the two masks (2)
mark_clear_bytes = 8 * NP
resolve_bytes = (8 + 3 + 12 + 2) * NP
copy_resolve_gbs, copy_resolve_ms = copy_gbs(resolve_bytes)
res = {"config": a.config, "tone_mapping": a.tone_mapping, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "views": s.n_views,
       "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "unseen_faces": int((labels == 0).sum()),
       "adjustments": "the library's global seam leveling (iterations %s)" % gst["iterations"],
       "runs": a.runs, "ms_median": med, "ms_runs": [{k: r[k] for k in phases} for r in runs],
       **{k: last[k] for k in ("patches", "merged", "listed_faces", "degenerate_faces", "pixels", "valid_pixels", "near_pixels")},
       "valid_share": last["valid_pixels"] / max(NP, 1), "near_share": last["near_pixels"] / max(NP, 1),
       "result_bytes": 14 * NP, "scratch_bytes": 8 * NP,
       "resolve": {"bytes": resolve_bytes, "gb_per_s": resolve_bytes / (med["ms_resolve"] * 1e-3) / 1e9 if med["ms_resolve"] > 0 else None,
                   "device_copy_same_bytes_gb_per_s": copy_resolve_gbs, "device_copy_same_bytes_ms": copy_resolve_ms},
       "mark": {"clear_bytes": mark_clear_bytes, "gb_per_s_clear_only": mark_clear_bytes / (med["ms_mark"] * 1e-3) / 1e9 if med["ms_mark"] > 0 else None},
       "note": "device time per phase from events on the context's stream (tables = components, boxes, merges, patch ids; lists = frames, "
               "the three scans, list entries and texture coordinates; mark = clearing the winner words + the two mark kernels; resolve = one "
               "thread per pixel: winner, crop + adjustment, masks -- the crop is fused into resolve, there is no separate crop pass); "
               "wall_ms = host clock around the call incl. input upload; outputs stay on the device"}
print(json.dumps({k: res[k] for k in ("ms_median", "patches", "merged", "pixels", "valid_share", "resolve", "mark")}), flush=True)

if not a.no_model:
    import patch_model as PM
    t = time.perf_counter()
    stm, want, wst, _ = PM.run_scene(s, labels, ca)
    res["model_single_thread_s"] = time.perf_counter() - t
    P = last["patches"]
    small = {"label": (np.uint32, P), "box": (np.int32, 4 * P), "face_ptr": (np.uint32, P + 1), "faces": (np.uint32, last["listed_faces"]),
             "texcoords": (np.float32, 6 * last["listed_faces"]), "pix_ptr": (np.uint64, P + 1)}
    ok = stm == 0 and all(last[k] == wst[k] for k in ("patches", "merged", "listed_faces", "degenerate_faces", "pixels", "valid_pixels", "near_pixels"))
    for k, (dt, n) in small.items():
        h = dev_bytes(got[k], n * np.dtype(dt).itemsize).view(dt)
        ok = ok and h.size == want[k].size and np.array_equal(h.view(np.uint8), want[k].view(np.uint8))
    pp = want["pix_ptr"].astype(np.int64)
    if a.window and P:
        pick = sorted(set([0, int(np.argmax(np.diff(pp)))] + [int(i) for i in np.linspace(0, P - 1, a.window)]))
        spans = [(int(pp[i]), int(pp[i + 1])) for i in pick]
    else:
        pick = "all"; spans = [(0, int(pp[-1]))] if P else []
    compared = 0
    for lo, hi in spans:
        for k, per in (("image", 12), ("validity", 1), ("blending", 1)):
            h = dev_bytes(got[k], (hi - lo) * per, lo * per)
            ok = ok and np.array_equal(h, want[k][lo * (per // want[k].itemsize):hi * (per // want[k].itemsize)].view(np.uint8))
        compared += hi - lo
    res["model_equal"] = bool(ok); res["model_compared_patches"] = pick if pick == "all" else len(pick); res["model_compared_pixels"] = compared
    print("model: %.1f s single thread, equal: %s (%s patches, %d pixels compared)" % (res["model_single_thread_s"], res["model_equal"], res["model_compared_patches"], compared), flush=True)
c.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
