"""View input at a BASELINE config, PNG files: the views saved by Pillow at its default compression (the rows per filter type it chose
are recorded) and brought into a context by either route:
   png_decode_time.py --config 3 [--runs 3] [--out profiles/pngdec_c3.json]
In one process on one box the two legs alternate, and the medians of the timed runs after one warm-up are recorded:
   host    today's route: Pillow decodes the files on 16 host threads, then set_views uploads the pixels (both parts reported);
   device  set_views_files: the IDAT payloads go up, one wave per file inflates, the Adler-32 is summed, one wave per file unfilters
           (per-stage device times from the stats).
Beside them the bytes either route uploads, the inflate rate per wave in MB/s of output (the mean file's inflated bytes over the mean
batch's inflate time: the waves of a batch run side by side), and the single-view case: one file through decode_pngs.  The last device run's pixels are compared with Pillow's.  The images are synthetic renders;
photographs compress less."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "tools")]
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "pngdec_c%d.json" % a.config)

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])


def encode(img):
    f = io.BytesIO()
    Image.fromarray(img).save(f, "PNG")
    return f.getvalue()


def decode(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8))


with ThreadPoolExecutor(16) as pool:
    files = list(pool.map(encode, s.images))
raw_bytes = sum(int(img.size) for img in s.images)
print("scene + %d files: %.1f s, %d pixel bytes, %d file bytes" % (len(files), time.perf_counter() - t0, raw_bytes, sum(map(len, files))), flush=True)

c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
host, device, single = [], [], []
for r in range(a.runs + 1):                    # run 0 is the warm-up: buffers, code objects, the pinned ring
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        pixels = list(pool.map(decode, files))
    t1 = time.perf_counter()
    c.set_views(s.cams, pixels)
    t2 = time.perf_counter()
    st = c.set_views_files(s.cams, files)["png"]
    t3 = time.perf_counter()
    one = decode(files[0])
    t4 = time.perf_counter()
    _, st1 = c.decode_pngs(files[:1])
    t5 = time.perf_counter()
    if r:
        host.append({"pillow_16_threads_ms": 1e3 * (t1 - t), "set_views_ms": 1e3 * (t2 - t1)})
        st["wall_ms"] = 1e3 * (t3 - t2)
        device.append(st)
        st1["wall_ms"] = 1e3 * (t5 - t4); st1["pillow_ms"] = 1e3 * (t4 - t3)
        single.append(st1)
    print("run %d: pillow %.0f ms, set_views %.0f ms, set_views_files %.0f ms (inflate %.0f ms)" % (r, 1e3 * (t1 - t), 1e3 * (t2 - t1), 1e3 * (t3 - t2), st["ms_inflate"]), flush=True)
got, _ = c.decode_pngs(files[:8])
equal = all(np.array_equal(x, y) for x, y in zip(got, pixels[:8]))
c.close()

med = lambda rows, k: float(np.median([r[k] for r in rows]))
last, last1 = device[-1], single[-1]
per_wave = lambda d: d["raw_bytes"] / max(d["files"], 1) * d["batches"] / max(d["ms_inflate"], 1e-6) / 1e3   # every file of a batch has a wave of its own
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "views": s.n_views, "runs": a.runs,
       "files": "Pillow PNG, default compression; synthetic renders (photographs compress less)",
       "host_route": {"pillow_16_threads_ms": med(host, "pillow_16_threads_ms"), "set_views_ms": med(host, "set_views_ms"), "bytes_uploaded": raw_bytes, "runs": host},
       "device_route": dict({k: med(device, k) for k in M.viewsel.PNGDEC_MS + ("wall_ms",)}, bytes_uploaded=last["zlib_bytes"], wall_ms_runs=[d["wall_ms"] for d in device],
                            filter_rows=last["filter_rows"], batches=last["batches"], **{k: last[k] for k in M.viewsel.PNGDEC_COUNTS}),
       "inflate_MB_per_s_per_wave": per_wave({k: (med(device, k) if k == "ms_inflate" else last[k]) for k in ("raw_bytes", "files", "batches", "ms_inflate")}),
       "single_view": dict({k: med(single, k) for k in M.viewsel.PNGDEC_MS + ("wall_ms", "pillow_ms")}, raw_bytes=last1["raw_bytes"], zlib_bytes=last1["zlib_bytes"],
                           inflate_MB_per_s=last1["raw_bytes"] / max(med(single, "ms_inflate"), 1e-6) / 1e3),
       "first_8_views_equal_pillow": bool(equal),
       "note": "legs alternate in one process; medians of the timed runs after one warm-up.  host clock around each part; ms_* are device times from events on the "
               "context's stream.  No pass mark: this is what was measured"}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
print("wrote", out_path)
