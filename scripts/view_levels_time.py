"""View input at a pyramid level, at a BASELINE config: the config's images are taken as the photographs (the SOURCES), the cameras are
scaled to the level's size, and the views are brought into a context at levels 1 and 2 by four routes:
   view_levels_time.py --config 3 [--runs 3] [--out profiles/view_levels_c3.json]
In one process on one box the legs alternate, and the medians of the timed runs after one warm-up are recorded:
   a  the host twin (halve_host) on 16 threads, then set_views uploads the level images;
   b  set_views(levels=): the pixels go up once, one launch halves them into the image buffers;
   c  files (quality 90, 4:2:0 JPEG): Pillow decodes on 16 host threads, then a;
   d  set_views_files(levels=): the entropy data goes up, the device decodes into staging and halves.
Also: the level kernel's device time without and with a lens (k2k4) from the events around its launch, beside a device copy of the
source bytes timed in the same process -- the kernel reads them once and writes a quarter or a sixteenth; the image bytes that stay
resident; and the data-cost pass at levels 0, 1 and 2.  View 0 and the last view of legs b and d are compared with leg a's / c's image.
The images are synthetic renders.  No pass mark is set."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "view_levels_c%d.json" % a.config)

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
V = s.n_views
raw_bytes = sum(int(img.size) for img in s.images)
flen = [float(s.cams["K"][j][0]) / max(int(s.cams["width"][j]), int(s.cams["height"][j])) for j in range(V)]


def cams_at(level):
    """the scene's cameras with the calibration of the level's size (the principal point and the focal lengths scale with the image)"""
    c = {k: np.array(v, copy=True) for k, v in s.cams.items()}
    for j in range(V):
        w, h = int(s.cams["width"][j]), int(s.cams["height"][j])
        wl, hl = M.level_size(w, h, level)
        K = c["K"][j].reshape(3, 3)
        K[0] *= np.float32(wl) / np.float32(w); K[1] *= np.float32(hl) / np.float32(h)
        c["width"][j], c["height"][j] = wl, hl
    return c


from PIL import Image  # noqa: E402
import torch  # noqa: E402


def encode(img):
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", quality=90, subsampling=2)
    return f.getvalue()


def decode(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8))


with ThreadPoolExecutor(16) as pool:
    files = list(pool.map(encode, s.images))
print("scene + %d files: %.1f s, %d pixel bytes, %d file bytes" % (V, time.perf_counter() - t0, raw_bytes, sum(map(len, files))), flush=True)

med = lambda rows, k: float(np.median([r[k] for r in rows]))
c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "views": V, "runs": a.runs, "source_bytes": raw_bytes,
       "file_bytes": sum(map(len, files)), "files": "Pillow JPEG, quality 90, 4:2:0; synthetic renders", "levels": {}}


def route_a(pixels, level, cams):
    with ThreadPoolExecutor(16) as pool:
        halved = list(pool.map(lambda p: M.halve_host(p, level), pixels))
    t = time.perf_counter()
    c.set_views(cams, halved)
    return halved, time.perf_counter() - t


def data_costs_ms(cams, images, levels):
    out = []
    for r in range(a.runs + 1):
        c.set_views(cams, images, levels=levels)
        c.synchronize()
        t = time.perf_counter()
        st = c.data_costs(M.Settings())
        c.synchronize()
        if r:
            out.append(1e3 * (time.perf_counter() - t))
    return float(np.median(out)), int(st["nnz"])


dc0, nnz0 = data_costs_ms(s.cams, s.images, None)
res["level_0"] = {"resident_image_bytes": raw_bytes, "data_costs_ms": dc0, "nnz": nnz0}
for level in (1, 2):
    cams = cams_at(level)
    rows = []
    equal_b = equal_d = None
    for r in range(a.runs + 1):                    # run 0 is the warm-up: buffers, code objects, the pinned ring
        t = time.perf_counter()
        halved, t_set = route_a(s.images, level, cams)
        t1 = time.perf_counter()
        st_b = c.set_views(cams, s.images, levels=level)
        t2 = time.perf_counter()
        if r == a.runs:
            equal_b = bool(np.array_equal(c.view_image(0), halved[0]) and np.array_equal(c.view_image(V - 1), halved[V - 1]))
        t3 = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            pixels = list(pool.map(decode, files))
        t4 = time.perf_counter()
        halved_c, _ = route_a(pixels, level, cams)
        t5 = time.perf_counter()
        st_d = c.set_views_files(cams, files, levels=level)
        t6 = time.perf_counter()
        if r == a.runs:
            equal_d = bool(np.array_equal(c.view_image(0), halved_c[0]) and np.array_equal(c.view_image(V - 1), halved_c[V - 1]))
        st_l = c.set_views(cams, s.images, levels=level, lens=np.array([(flen[j], -0.2, 0.05) for j in range(V)], np.float32))
        if r:
            rows.append({"a_ms": 1e3 * (t1 - t), "a_set_views_ms": 1e3 * t_set, "b_ms": 1e3 * (t2 - t1), "b_ms_upload": st_b["level"]["ms_upload"], "kernel_ms": st_b["level"]["ms_halve"],
                         "kernel_batches": st_b["level"]["batches"], "c_ms": 1e3 * (t5 - t3), "c_pillow_ms": 1e3 * (t4 - t3), "d_ms": 1e3 * (t6 - t5), "d_kernel_ms": st_d["level"]["ms_halve"],
                         "d_ms_decode_stages": sum(st_d["jpeg"][k] for k in M.viewsel.JPEGDEC_MS), "d_jpeg_batches": st_d["jpeg"]["batches"], "d_level_batches": st_d["level"]["batches"],
                         "kernel_with_lens_ms": st_l["level"]["ms_halve"], "pixels_no_source": st_l["lens"]["pixels_no_source"], "staging_bytes": st_b["level"]["staging_bytes"]})
        del halved, halved_c, pixels
    dc, nnz = data_costs_ms(cams, s.images, level)
    resident = int(st_b["level"]["pixels_out"]) * 3
    res["levels"][str(level)] = dict({k: med(rows, k) for k in rows[0]}, runs=rows, b_views_equal_a=equal_b, d_views_equal_c=equal_d, resident_image_bytes=resident,
                                     data_costs_ms=dc, nnz=nnz)
c.close()
x = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
y.copy_(x); torch.cuda.synchronize()
copies = []
for _ in range(a.runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
    copies.append(float(e0.elapsed_time(e1)))
del x, y
res["device_copy_of_the_source_ms"] = float(np.median(copies))
for level in res["levels"].values():
    level["kernel_over_copy"] = level["kernel_ms"] / res["device_copy_of_the_source_ms"]
    level["kernel_read_GBps"] = raw_bytes / level["kernel_ms"] / 1e6
res["note"] = ("legs alternate in one process; medians of the timed runs after one warm-up; host clock around each leg, kernel_ms are device times from events on the "
               "context's stream around the level launches (summed over the batches).  The copy reads and writes the source bytes once each; the kernel reads them "
               "once and writes a quarter (level 1) or a sixteenth (level 2).  Legs a and c are the host routes, not compared against a bound")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: {a_: b_ for a_, b_ in d.items() if a_ != "runs"} for k, d in res["levels"].items()}, indent=1))
print("level 0", res["level_0"], "device copy ms", res["device_copy_of_the_source_ms"])
print("wrote", out_path)
