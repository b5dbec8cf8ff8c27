"""The JPEG route of rows f9 / f11 at a BASELINE config, with labels from the library's own view selection and rows f5 - f8 left on the device:
   jpeg_output_time.py --config 3 [--runs 3] [--out profiles/jpeg_c3.json]
In one process on one box, save_model and save_glb run alternately under png_device = 1 and under image_format = 1 (quality 90, 4:2:0 and
4:4:4), and the medians of the timed runs after one warm-up are recorded: ms_png and the image bytes of both calls per leg.  Then
Context.encode_jpegs and Context.encode_pngs on the same atlases: the device time per pass, the segment pass beside png_chunk_kernel
(ms per raw megabyte) and beside a device-to-device copy of the same raw bytes timed in the same run, and the share of marker and
stuffing bytes in the files.  Every file of the last run is opened with Pillow and the sizes it reports are recorded."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
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
out_path = a.out or os.path.join(ROOT, "profiles", "jpeg_c%d.json" % a.config)

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
c.set_views(s.cams, s.images)
c.data_costs(M.Settings())
labels, ms = c.view_selection(s.adj_ptr, s.adj)
gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, on_device=True)
dev, pst = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], on_device=True)
lsl, _ = c.local_seam_leveling(s.adj_ptr, s.adj, labels, dev, on_device=True)
dev = dict(dev); dev.update(image=lsl["image"], validity=lsl["validity"])
atl, ast = c.texture_atlases(dev, on_device=True)
dn = torch.from_numpy(M.vertex_normals(s.verts, s.faces)).cuda()
torch.cuda.synchronize()
print("scene + labels + rows f5 - f8: %.1f s, %d faces, %d atlases, %d atlas pixels" % (time.perf_counter() - t0, s.n_faces, ast["atlases"], ast["pixels"]), flush=True)

name = "jpeg_c%d" % a.config
med = lambda rows, k: float(np.median([r[k] for r in rows]))
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "views": s.n_views,
       "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "atlases": ast["atlases"], "atlas_pixels": ast["pixels"], "raw_bytes": 3 * ast["pixels"],
       "runs": a.runs, "legs": {}, "passes": {},
       "note": "save_model and save_glb alternate leg by leg in one process, atlases and normals on the device; medians of the timed runs after one warm-up of each.  "
               "ms_png: host clock around the images of the call (encode, download, framing; save_model: the files as well); device times from events on the context's stream"}
LEGS = (("png_device", dict(png_device=1)), ("jpeg_q90_420", dict(image_format="jpeg", jpeg_quality=90, jpeg_subsampling=1)),
        ("jpeg_q90_444", dict(image_format="jpeg", jpeg_quality=90, jpeg_subsampling=0)))
tmp = tempfile.mkdtemp(prefix="jpeg_output_")
try:
    runs = {leg: {"model": [], "glb": []} for leg, _ in LEGS}
    for r in range(a.runs + 1):                                # run 0 is the warm-up: buffers, code objects, the pinned buffer, the page cache
        for leg, kw in LEGS:
            p = M.default_model_params(**kw)
            d = os.path.join(tmp, leg)
            os.makedirs(d, exist_ok=True)
            prefix = os.path.join(d, name)
            t = time.perf_counter(); so = c.save_model(atl, prefix, dn, p); so["wall_ms"] = 1e3 * (time.perf_counter() - t)
            t = time.perf_counter(); sg = c.save_glb(atl, prefix + ".glb", dn, p); sg["wall_ms"] = 1e3 * (time.perf_counter() - t)
            if r:
                runs[leg]["model"].append(so); runs[leg]["glb"].append(sg)
    for leg, kw in LEGS:
        d = os.path.join(tmp, leg)
        size = {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)}
        ext = ".jpg" if "image_format" in kw else ".png"
        res["legs"][leg] = {"params": kw, "save_model_ms_png": med(runs[leg]["model"], "ms_png"), "save_model_wall_ms": med(runs[leg]["model"], "wall_ms"),
                            "save_glb_ms_png": med(runs[leg]["glb"], "ms_png"), "save_glb_wall_ms": med(runs[leg]["glb"], "wall_ms"),
                            "save_model_ms_png_runs": [x["ms_png"] for x in runs[leg]["model"]], "save_glb_ms_png_runs": [x["ms_png"] for x in runs[leg]["glb"]],
                            "image_files_bytes": sum(v for f, v in size.items() if f.endswith(ext)), "glb_image_bytes": runs[leg]["glb"][-1]["image_bytes"],
                            "glb_file_bytes": size[name + ".glb"]}
        print(leg, json.dumps(res["legs"][leg]), flush=True)
    # ---- the passes on their own ----
    raw = 3 * ast["pixels"]
    x = torch.empty(raw, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
    y.copy_(x); torch.cuda.synchronize()
    c.encode_pngs(atl)
    for sub in (1, 0):
        c.encode_jpegs(atl, 90, sub)
    png_rows, copies, jpeg_rows, last = [], [], {1: [], 0: []}, {}
    for _ in range(a.runs):
        png_rows.append(c.encode_pngs(atl)[1])
        for sub in (1, 0):
            files, st = c.encode_jpegs(atl, 90, sub)
            jpeg_rows[sub].append(st)
            last[sub] = files
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
        copies.append(float(e0.elapsed_time(e1)))
    del x, y
    copy_ms = float(np.median(copies))
    chunk_ms = med(png_rows, "ms_chunk")
    res["passes"]["png_device"] = {k: med(png_rows, k) for k in M.viewsel.PNG_MS}
    res["passes"]["png_device"].update(raw_bytes=png_rows[-1]["raw_bytes"], png_bytes=png_rows[-1]["png_bytes"], chunk_ms_per_raw_mb=chunk_ms / (png_rows[-1]["raw_bytes"] / 1e6))
    res["passes"]["device_copy_ms"] = copy_ms
    from PIL import Image
    for sub in (1, 0):
        st = jpeg_rows[sub][-1]
        row = {k: med(jpeg_rows[sub], k) for k in M.viewsel.JPEG_MS}
        row.update({k: st[k] for k in M.viewsel.JPEG_COUNTS})
        row.update(segment_ms_per_raw_mb=row["ms_segment"] / (st["raw_bytes"] / 1e6), segment_over_png_chunk=row["ms_segment"] / chunk_ms if chunk_ms > 0 else None,
                   segment_over_device_copy=row["ms_segment"] / copy_ms if copy_ms > 0 else None, segment_gb_per_s=st["raw_bytes"] / (row["ms_segment"] * 1e-3) / 1e9,
                   marker_share=st["marker_bytes"] / st["jpeg_bytes"], stuffing_share=st["stuffed_bytes"] / st["jpeg_bytes"],
                   rst_marker_share=2 * (st["segments"] - ast["atlases"]) / st["jpeg_bytes"], compression=st["raw_bytes"] / st["jpeg_bytes"])
        sizes = sorted(set(Image.open(io.BytesIO(f)).size for f in last[sub]))
        row["decoded_sizes"] = [list(v) for v in sizes]
        res["passes"]["jpeg_q90_%s" % ("420" if sub else "444")] = row
        print("jpeg sub %d" % sub, json.dumps(row), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
c.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
