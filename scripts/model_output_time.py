"""Row f9 (model output) at a BASELINE config, with labels from the library's own view selection and rows f5 - f8 left on the device:
   model_output_time.py --config 3 [--runs 3] [--out profiles/model_c3.json] [--no-model] [--png-levels 0,1,6] [--png-device]
Records, as the median of the timed runs after one warm-up: the device time per phase of the text (mvs_model_stats ms_measure / ms_scan /
ms_write, from events on the context's stream; inputs and the text stay on the device), a plain device-to-device copy of obj_bytes timed
in the same run -- the bound the write kernel is compared against -- and their ratio; the host times of save_model per PNG level
(ms_download: the text through the pinned buffer, ms_files: the two text files, ms_png: atlas pixels to the host, encoding on up to 16
threads, writing); the lines and bytes per section and the wide-route / non-finite counters; and the single-thread time of the CPU model
(tests/tools/obj_model.cpp: std::ostringstream << std::fixed) on the same inputs, with the .obj and .mtl files compared in full.
--png-device adds a leg with params.png_device = 1 (the PNGs compressed on the device) under the same keys, and beside it the stats of
Context.encode_pngs on the same atlases: the device time of the filter, chunk and gather passes, their GB/s on the raw bytes next to a
device copy of that many bytes, the host time of the download and the framing, chunks and stored chunks, rows per filter type."""
import argparse
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
ap.add_argument("--no-model", action="store_true")
ap.add_argument("--png-levels", default="0", help="comma-separated png_level values to time save_model with")
ap.add_argument("--png-device", action="store_true", help="also time save_model with png_device = 1 and Context.encode_pngs on the atlases")
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "model_c%d.json" % a.config)
levels = [int(x) for x in a.png_levels.split(",")]

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
normals = M.vertex_normals(s.verts, s.faces)
dn = torch.from_numpy(normals).cuda()
torch.cuda.synchronize()
print("scene + labels + rows f5 - f8: %.1f s, %d faces, %d vertices, %d atlases, %d atlas pixels" % (time.perf_counter() - t0, s.n_faces, len(s.verts), ast["atlases"], ast["pixels"]), flush=True)

name = "model_c%d" % a.config
c.build_model(atl, dn, name, on_device=True)             # warm-up: buffers, code objects
runs = []
for _ in range(a.runs):
    t = time.perf_counter()
    got, st = c.build_model(atl, dn, name, on_device=True)
    st["wall_ms"] = 1e3 * (time.perf_counter() - t)
    runs.append(st)
phases = ("ms_measure", "ms_scan", "ms_write", "wall_ms")
med = {k: float(np.median([r[k] for r in runs])) for k in phases}
last = runs[-1]
obj_bytes = int(sum(last["bytes"].values()))
x = torch.empty(obj_bytes, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
y.copy_(x); torch.cuda.synchronize()
copies = []
for _ in range(a.runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
    copies.append(float(e0.elapsed_time(e1)))
del x, y
copy_ms = float(np.median(copies))
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "vertices": int(len(s.verts)), "views": s.n_views,
       "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "atlases": ast["atlases"], "atlas_pixels": ast["pixels"], "runs": a.runs,
       "lines": last["lines"], "bytes": last["bytes"], "obj_bytes": obj_bytes, "mtl_bytes": last["mtl_bytes"], "wide_values": last["wide_values"],
       "nonfinite_values": last["nonfinite_values"], "ms_median": med, "ms_runs": [{k: r[k] for k in phases} for r in runs],
       "write": {"gb_per_s": obj_bytes / (med["ms_write"] * 1e-3) / 1e9 if med["ms_write"] > 0 else None, "device_copy_obj_bytes_ms": copy_ms,
                 "device_copy_gb_per_s": obj_bytes / (copy_ms * 1e-3) / 1e9 if copy_ms > 0 else None, "write_over_copy": med["ms_write"] / copy_ms if copy_ms > 0 else None},
       "note": "ms_measure / ms_scan / ms_write: device time from events on the context's stream, atlases, normals and text on the device; wall_ms: host clock around "
               "build_model; device_copy: a device-to-device copy of obj_bytes (reads and writes that many bytes; the write kernel reads the ~16 B per line of its inputs "
               "and the 8-byte offsets and writes obj_bytes)"}
print(json.dumps({k: res[k] for k in ("ms_median", "lines", "bytes", "write", "wide_values")}), flush=True)

tmp = tempfile.mkdtemp(prefix="model_output_")
try:
    res["save_model"] = {}
    legs = [("png_level_%d" % level, "l%d" % level, dict(png_level=level)) for level in levels] + ([("png_device", "dev", dict(png_device=1))] if a.png_device else [])
    for leg, sub, kw in legs:
        p = M.default_model_params(**kw)
        prefix = os.path.join(tmp, sub, name)
        os.makedirs(os.path.dirname(prefix))
        c.save_model(atl, prefix, dn, p)                  # warm-up: the pinned buffer, the page cache
        sr = []
        for _ in range(a.runs):
            t = time.perf_counter()
            st = c.save_model(atl, prefix, dn, p)
            st["wall_ms"] = 1e3 * (time.perf_counter() - t)
            sr.append(st)
        keys = ("ms_download", "ms_files", "ms_png", "wall_ms")
        png_bytes = sum(os.path.getsize(os.path.join(os.path.dirname(prefix), f)) for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".png"))
        res["save_model"][leg] = {"ms_median": {k: float(np.median([r[k] for r in sr])) for k in keys}, "png_bytes": int(png_bytes), "threads": min(16, ast["atlases"])}
        print("save_model %s: %s, %d PNG bytes" % (leg, json.dumps(res["save_model"][leg]["ms_median"]), png_bytes), flush=True)
    if a.png_device:
        c.encode_pngs(atl)                                # warm-up
        er = []
        for _ in range(a.runs):
            t = time.perf_counter()
            _, st = c.encode_pngs(atl)
            st["wall_ms"] = 1e3 * (time.perf_counter() - t)
            er.append(st)
        raw = er[-1]["raw_bytes"]
        x = torch.empty(raw, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
        y.copy_(x); torch.cuda.synchronize()
        copies = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
            copies.append(float(e0.elapsed_time(e1)))
        del x, y
        keys = ("ms_filter", "ms_chunk", "ms_gather", "ms_download", "ms_frame", "wall_ms")
        emed = {k: float(np.median([r[k] for r in er])) for k in keys}
        raw_copy_ms = float(np.median(copies))
        res["encode_pngs"] = {"ms_median": emed, "raw_bytes": raw, "png_bytes": er[-1]["png_bytes"], "chunks": er[-1]["chunks"], "stored_chunks": er[-1]["stored_chunks"],
                              "filter_rows": er[-1]["filter_rows"], "device_copy_raw_bytes_ms": raw_copy_ms,
                              "gb_per_s": {k: raw / (emed[k] * 1e-3) / 1e9 if emed[k] > 0 else None for k in ("ms_filter", "ms_chunk", "ms_gather")},
                              "device_copy_gb_per_s": raw / (raw_copy_ms * 1e-3) / 1e9 if raw_copy_ms > 0 else None,
                              "note": "Context.encode_pngs on the device-resident atlases; GB/s on raw_bytes = the filtered streams"}
        print("encode_pngs: %s" % json.dumps(res["encode_pngs"]), flush=True)
    if not a.no_model:
        import obj_model as OM
        OM.build()

        def dev_host(d, dtype):
            dt = np.dtype(dtype); n = d.shape[0]
            if n == 0:
                return np.zeros(0, dt)

            class _Dev:
                __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (d.data_ptr(), False), "version": 2}
            return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt)
        host = {k: dev_host(atl[k], dt) for k, dt in (("face_ptr", np.uint32), ("faces", np.uint32), ("tc_ptr", np.uint32), ("texcoords_merged", np.float32),
                                                       ("texcoord_ids", np.uint32))}
        OM.load()
        t = time.perf_counter()
        want_obj, want_mtl = OM.run(s.verts, s.faces, host, normals, name)
        res["model_single_thread_s"] = time.perf_counter() - t
        prefix = os.path.join(tmp, legs[0][1], name)
        with open(prefix + ".obj", "rb") as f:
            obj_equal = f.read() == want_obj
        with open(prefix + ".mtl", "rb") as f:
            mtl_equal = f.read() == want_mtl
        res["model_equal"] = bool(obj_equal and mtl_equal)
        res["model_over_device_text"] = res["model_single_thread_s"] * 1e3 / (med["ms_measure"] + med["ms_scan"] + med["ms_write"])
        print("model: %.2f s single thread (text in memory, no file), files equal: %s" % (res["model_single_thread_s"], res["model_equal"]), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
c.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
