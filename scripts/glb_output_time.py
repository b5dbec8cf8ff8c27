"""Row f11 (binary glTF output) at a BASELINE config, with labels from the library's own view selection and rows f5 - f8 left on the device:
   glb_output_time.py --config 3 [--runs 3] [--out profiles/glb_c3.json] [--no-check]
In one process on one box, save_glb and save_model run alternately with the same mvs_model_params (one leg with the default, one with
png_device = 1), and the medians of the timed runs after one warm-up are recorded: the device time per phase of row f11 (keys, sort,
number, indices, gather; events on the context's stream), its host times (PNGs, download, file) and the wall clock of both calls; the
number of glTF vertices NP; the .glb's bytes beside the .obj + .mtl bytes and beside everything save_model writes; and the gather pass's
bytes per second (the attribute bytes it writes) beside a device-to-device copy of that many bytes timed in the same run.  Unless
--no-check, the file is parsed (tests/tools/glb_model.py), its BIN chunk and JSON are compared with the numpy restatement, and its
embedded PNGs with the files save_model wrote.
   glb_output_time.py --config 3 --quantize [--out profiles/glb_quant_c3.json]
runs the leg of glb_quantize = 1 (DESIGN.md section 4 "Model output" item 10) instead: save_glb with glb_quantize 1 and with 0 alternate in
one process with the same image parameters (JPEG at the defaults), and the medians of the timed runs are recorded for both: the file's and
the geometry's bytes, the device phases (ms_bounds among them), the gather's bytes per second beside a device copy of as many bytes, and
the ratio of the two gathers.  Unless --no-check the quantised file is parsed (tests/tools/glb_quant_model.py) and compared with the
restatement."""
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
ap.add_argument("--no-check", action="store_true")
ap.add_argument("--quantize", action="store_true", help="the glb_quantize = 1 leg beside the float route (profiles/glb_quant_c<config>.json)")
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", ("glb_quant_c%d.json" if a.quantize else "glb_c%d.json") % a.config)

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

name = "glb_c%d" % a.config
GLB_KEYS = M.viewsel.GLB_MS + M.viewsel.GLB_QUANT_MS + ("wall_ms",)
OBJ_KEYS = M.viewsel.MODEL_MS + ("wall_ms",)
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "vertices": int(len(s.verts)), "views": s.n_views,
       "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "atlases": ast["atlases"], "atlas_pixels": ast["pixels"], "runs": a.runs, "legs": {},
       "note": "save_glb and save_model alternate in one process, same mvs_model_params per leg, vertex normals given, atlases and normals on the device; medians "
               "of the timed runs after one warm-up of each.  ms_keys .. ms_gather: device time from events on the context's stream; ms_png / ms_download / ms_file "
               "(ms_files): host time; wall_ms: host clock around the call"}


def device_copy_ms(n_bytes):
    """median device time of a device-to-device copy of n_bytes"""
    x = torch.empty(n_bytes, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
    y.copy_(x); torch.cuda.synchronize()
    copies = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
        copies.append(float(e0.elapsed_time(e1)))
    return float(np.median(copies))


def host_atlases():
    def dev_host(darr, dtype):
        dt = np.dtype(dtype); n = darr.shape[0]
        if n == 0:
            return np.zeros(0, dt)

        class _Dev:
            __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (darr.data_ptr(), False), "version": 2}
        return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt)
    return {k: dev_host(atl[k], dt) for k, dt in (("face_ptr", np.uint32), ("faces", np.uint32), ("tc_ptr", np.uint32), ("texcoords_merged", np.float32), ("texcoord_ids", np.uint32))}


def quantize_leg(d):
    """save_glb with glb_quantize 1 and 0 alternately, the same JPEG parameters: the medians of both and the quantised file's check"""
    kw = dict(image_format=1)
    params = {"quantized": M.default_model_params(glb_quantize=1, **kw), "float": M.default_model_params(glb_quantize=0, **kw)}
    path = {k: os.path.join(d, "%s_%s.glb" % (name, k)) for k in params}
    for k in params:
        c.save_glb(atl, path[k], dn, params[k])                     # warm-up
    runs = {k: [] for k in params}
    for _ in range(a.runs):
        for k in params:
            t = time.perf_counter(); st = c.save_glb(atl, path[k], dn, params[k]); st["wall_ms"] = 1e3 * (time.perf_counter() - t); runs[k].append(st)
    leg = {"params": kw}
    for k in params:
        last = runs[k][-1]
        med = {m: float(np.median([r[m] for r in runs[k]])) for m in GLB_KEYS}
        idx_bytes = 4 * last["indices"] if k == "float" else last["geometry_bytes"] - (16 if normals is not None else 12) * last["vertices"]
        attr_bytes = last["geometry_bytes"] - idx_bytes
        copy_ms = device_copy_ms(attr_bytes)
        leg[k] = {"save_glb_ms_median": med, "save_glb_ms_runs": [{m: r[m] for m in GLB_KEYS} for r in runs[k]], "NP": last["vertices"], "indices": last["indices"],
                  "primitives": last["primitives"], "index16_primitives": last["index16_primitives"], "zero_normals": last["zero_normals"],
                  "glb": {m: last[m] for m in ("json_bytes", "geometry_bytes", "image_bytes", "file_bytes")}, "index_bytes": idx_bytes, "file_on_disk": os.path.getsize(path[k]),
                  "gather": {"attribute_bytes": attr_bytes, "gb_per_s": attr_bytes / (med["ms_gather"] * 1e-3) / 1e9 if med["ms_gather"] > 0 else None, "device_copy_ms": copy_ms,
                             "device_copy_gb_per_s": attr_bytes / (copy_ms * 1e-3) / 1e9 if copy_ms > 0 else None, "gather_over_copy": med["ms_gather"] / copy_ms if copy_ms > 0 else None}}
    q, f = leg["quantized"], leg["float"]
    leg["quantized_over_float"] = {"file_bytes": q["glb"]["file_bytes"] / f["glb"]["file_bytes"], "geometry_bytes": q["glb"]["geometry_bytes"] / f["glb"]["geometry_bytes"],
                                   "ms_gather": q["save_glb_ms_median"]["ms_gather"] / f["save_glb_ms_median"]["ms_gather"],
                                   "ms_bounds_plus_gather_over_float_gather": (q["save_glb_ms_median"]["ms_bounds"] + q["save_glb_ms_median"]["ms_gather"]) / f["save_glb_ms_median"]["ms_gather"],
                                   "ms_indices": q["save_glb_ms_median"]["ms_indices"] / f["save_glb_ms_median"]["ms_indices"], "wall_ms": q["save_glb_ms_median"]["wall_ms"] / f["save_glb_ms_median"]["wall_ms"]}
    print("quantize", json.dumps({k: leg[k] for k in ("quantized_over_float",)}), json.dumps({k: {m: leg[k][m] for m in ("save_glb_ms_median", "glb", "gather")} for k in params}), flush=True)
    if not a.no_check:
        import glb_quant_model as QM
        t = time.perf_counter()
        with open(path["quantized"], "rb") as fh:
            got = QM.parse_glb(fh.read())
        want = QM.restate(s.verts, s.faces, host_atlases(), normals, got["images"], "image/jpeg")
        leg["file_equals_restatement"] = bool(got["bin"] == want["bin"] and QM.json_equal(got["json"], want["json"]))
        print("quantize: parsed and compared with the numpy restatement in %.1f s: %s" % (time.perf_counter() - t, leg["file_equals_restatement"]), flush=True)
    return leg


def write_result():
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


tmp = tempfile.mkdtemp(prefix="glb_output_")
if a.quantize:
    try:
        res["legs"]["quantize"] = quantize_leg(tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    c.close()
    write_result()
    sys.exit(0)
try:
    for leg, kw in (("png_level_0", dict()), ("png_device", dict(png_device=1))):
        p = M.default_model_params(**kw)
        d = os.path.join(tmp, leg)
        os.makedirs(d)
        prefix = os.path.join(d, name)
        c.save_glb(atl, prefix + ".glb", dn, p); c.save_model(atl, prefix, dn, p)      # warm-up: buffers, code objects, the pinned buffer, the page cache
        gr, orr = [], []
        for _ in range(a.runs):
            t = time.perf_counter(); st = c.save_glb(atl, prefix + ".glb", dn, p); st["wall_ms"] = 1e3 * (time.perf_counter() - t); gr.append(st)
            t = time.perf_counter(); so = c.save_model(atl, prefix, dn, p); so["wall_ms"] = 1e3 * (time.perf_counter() - t); orr.append(so)
        size = {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)}
        last = gr[-1]
        gmed = {k: float(np.median([r[k] for r in gr])) for k in GLB_KEYS}
        omed = {k: float(np.median([r[k] for r in orr])) for k in OBJ_KEYS}
        attr_bytes = last["geometry_bytes"] - 4 * last["indices"]
        copy_ms = device_copy_ms(attr_bytes)
        text_bytes = size[name + ".obj"] + size[name + ".mtl"]
        res["legs"][leg] = {
            "params": kw, "save_glb_ms_median": gmed, "save_model_ms_median": omed, "save_glb_ms_runs": [{k: r[k] for k in GLB_KEYS} for r in gr],
            "save_model_ms_runs": [{k: r[k] for k in OBJ_KEYS} for r in orr], "save_glb_over_save_model_wall": gmed["wall_ms"] / omed["wall_ms"],
            "NP": last["vertices"], "indices": last["indices"], "primitives": last["primitives"],
            "glb": {k: last[k] for k in ("json_bytes", "geometry_bytes", "image_bytes", "file_bytes")},
            "obj_bytes": size[name + ".obj"], "mtl_bytes": size[name + ".mtl"], "obj_plus_mtl_bytes": text_bytes,
            "png_files_bytes": sum(v for f, v in size.items() if f.endswith(".png")), "save_model_files": len(size) - 1,
            "geometry_over_text": last["geometry_bytes"] / text_bytes,
            "gather": {"attribute_bytes": attr_bytes, "gb_per_s": attr_bytes / (gmed["ms_gather"] * 1e-3) / 1e9 if gmed["ms_gather"] > 0 else None,
                       "device_copy_ms": copy_ms, "device_copy_gb_per_s": attr_bytes / (copy_ms * 1e-3) / 1e9 if copy_ms > 0 else None,
                       "gather_over_copy": gmed["ms_gather"] / copy_ms if copy_ms > 0 else None,
                       "note": "the gather writes attribute_bytes in file order and reads as many through 8-byte pair keys at random vertices; the copy reads and writes them in order"}}
        print(leg, json.dumps({k: res["legs"][leg][k] for k in ("save_glb_ms_median", "save_model_ms_median", "NP", "glb", "obj_plus_mtl_bytes", "gather")}), flush=True)
        if not a.no_check:
            import glb_model as GM
            host = host_atlases()
            t = time.perf_counter()
            with open(prefix + ".glb", "rb") as f:
                got = GM.parse_glb(f.read())
            pngs = []
            for i in range(ast["atlases"]):
                with open("%s_material%04d_map_Kd.png" % (prefix, i), "rb") as f:
                    pngs.append(f.read())
            want = GM.restate(s.verts, s.faces, host, normals, pngs)
            ok = bool(got["bin"] == want["bin"] and GM.json_equal(got["json"], want["json"]) and got["images"] == pngs)
            res["legs"][leg]["file_equals_restatement"] = ok
            print("%s: parsed and compared with the numpy restatement in %.1f s: %s" % (leg, time.perf_counter() - t, ok), flush=True)
            del got, want, pngs
finally:
    shutil.rmtree(tmp, ignore_errors=True)
c.close()
write_result()
