"""View input of a scene whose cameras carry distortion coefficients, at a BASELINE config: every view gets the same lens -- k2k4 (-0.2, 0.05),
then VisualSFM (-0.12, 0) -- and is brought into a context by four routes:
   undistort_time.py --config 3 [--runs 3] [--out profiles/undistort_c3.json]
In one process on one box the legs alternate, and the medians of the timed runs after one warm-up are recorded:
   a  today's route for pixels: undistort_image per view (upload, undistort_kernel, download), then set_views uploads the result;
   b  set_views(lens=): the pixels go up once, one batched launch undistorts them into the image buffers;
   c  today's route for files (quality 90, 4:2:0 JPEG): Pillow decodes on 16 host threads, then a;
   d  set_views_jpeg(lens=): the entropy data goes up, the device decodes into staging and undistorts.
Kernel only: a child process under `rocprofv3 --kernel-trace --stats` runs a and b once more on the same images; the total of
undistort_kernel (one launch per image) stands against the total of lens_kernel (one per batch), beside a device copy of the same bytes.
View 0 of legs b and d is compared with leg a's / c's image.  The images are synthetic renders."""
import argparse
import csv
import glob
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

LENSES = {"k2k4": (-0.2, 0.05), "vsfm": (-0.12, 0.0)}

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--kernels-child", default=None, help="(internal) run legs a and b once for this lens model under the profiler")
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "undistort_c%d.json" % a.config)

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
V = s.n_views
flen = [float(s.cams["K"][j][0]) / max(int(s.cams["width"][j]), int(s.cams["height"][j])) for j in range(V)]
raw_bytes = sum(int(img.size) for img in s.images)


def lens_rows(model):
    return np.array([(flen[j],) + LENSES[model] for j in range(V)], np.float32)


def route_a(c, pixels, model):
    d0, d1 = LENSES[model]
    undist = [M.viewsel.undistort_image(pixels[j], flen[j], d0, d1) for j in range(V)]
    t = time.perf_counter()
    c.set_views(s.cams, undist)
    return undist, time.perf_counter() - t


if a.kernels_child:
    c = M.Context(0)
    c.set_mesh(s.verts, s.faces, s.normals)
    route_a(c, s.images, a.kernels_child)
    st = c.set_views(s.cams, s.images, lens=lens_rows(a.kernels_child))
    c.close()
    print("child: lens ms_undistort %.3f" % st["ms_undistort"])
    sys.exit(0)


def kernels_only(model):
    """total device time (ms) and launches of undistort_kernel and lens_kernel over the scene's images, from a kernel trace of a child"""
    tmp = tempfile.mkdtemp(prefix="mvs_lens_kt_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "kt", "--", sys.executable, os.path.abspath(__file__),
               "--config", str(a.config), "--kernels-child", model]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        out = {}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in ("undistort_kernel", "lens_kernel"):
                    if k in row["Name"]:
                        o = out.setdefault(k, {"launches": 0, "total_ms": 0.0}); o["launches"] += int(row["Calls"]); o["total_ms"] += float(row["TotalDurationNs"]) / 1e6
        if len(out) != 2:
            out["error"] = r.stdout[-600:]
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


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
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "views": V, "runs": a.runs, "pixel_bytes": raw_bytes,
       "file_bytes": sum(map(len, files)), "files": "Pillow JPEG, quality 90, 4:2:0; synthetic renders", "models": {}}
for model in LENSES:
    lens = lens_rows(model)
    rows = []
    equal_b = equal_d = None
    for r in range(a.runs + 1):                    # run 0 is the warm-up: buffers, code objects, the pinned ring
        t = time.perf_counter()
        undist, t_set = route_a(c, s.images, model)
        t1 = time.perf_counter()
        st_b = c.set_views(s.cams, s.images, lens=lens)
        t2 = time.perf_counter()
        if r == a.runs:
            equal_b = bool(np.array_equal(c.view_image(0), undist[0]) and np.array_equal(c.view_image(V - 1), undist[V - 1]))
        t3 = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            pixels = list(pool.map(decode, files))
        t4 = time.perf_counter()
        undist_c, _ = route_a(c, pixels, model)
        t5 = time.perf_counter()
        st_d = c.set_views_jpeg(s.cams, files, lens=lens)
        t6 = time.perf_counter()
        if r == a.runs:
            equal_d = bool(np.array_equal(c.view_image(0), undist_c[0]) and np.array_equal(c.view_image(V - 1), undist_c[V - 1]))
        if r:
            rows.append({"a_ms": 1e3 * (t1 - t), "a_set_views_ms": 1e3 * t_set, "b_ms": 1e3 * (t2 - t1), "b_ms_upload": st_b["ms_upload"], "b_ms_undistort": st_b["ms_undistort"],
                         "c_ms": 1e3 * (t5 - t3), "c_pillow_ms": 1e3 * (t4 - t3), "d_ms": 1e3 * (t6 - t5), "d_ms_undistort": st_d["lens"]["ms_undistort"],
                         "d_ms_decode_stages": sum(st_d[k] for k in M.viewsel.JPEGDEC_MS), "d_jpeg_batches": st_d["batches"], "d_lens_batches": st_d["lens"]["batches"],
                         "pixels_no_source": st_b["pixels_no_source"], "staging_bytes": st_b["staging_bytes"]})
        del undist, undist_c, pixels
    res["models"][model] = dict({k: med(rows, k) for k in rows[0]}, lens=list(LENSES[model]), runs=rows, b_views_equal_a=equal_b, d_views_equal_c=equal_d)
c.close()
x = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
y.copy_(x); torch.cuda.synchronize()
copies = []
for _ in range(a.runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
    copies.append(float(e0.elapsed_time(e1)))
del x, y
res["device_copy_of_the_pixels_ms"] = float(np.median(copies))
for model in LENSES:
    res["models"][model]["kernels_only"] = kernels_only(model)
res["note"] = ("legs alternate in one process; medians of the timed runs after one warm-up; host clock around each leg, ms_* are device times from events on the "
               "context's stream.  kernels_only: totals of a kernel trace of one more pass in a child process.  Legs a and c are the parent commit's routes, "
               "not compared against a bound")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({m: {k: v for k, v in d.items() if k != "runs"} for m, d in res["models"].items()}, indent=1))
print("device copy ms", res["device_copy_of_the_pixels_ms"])
print("wrote", out_path)
