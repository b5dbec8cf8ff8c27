"""View input at a BASELINE config: the views saved as Pillow JPEG (quality 90, 4:2:0, no restart markers -- how a camera writes them) and
brought into a context by either route:
   jpeg_decode_time.py --config 3 [--runs 3] [--out profiles/jpegdec_c3.json]
In one process on one box the two legs alternate, and the medians of the timed runs after one warm-up are recorded:
   host    today's route: Pillow decodes the files on 16 host threads, then set_views uploads the pixels (both parts reported);
   device  set_views_jpeg: the entropy data goes up, the device decodes (per-stage device times from the stats).
Beside them the bytes either route uploads, a device-to-device copy of the decoded bytes as the floor, and how the self-synchronising
decode behaved: subsequences exact after the first guess, the most rounds a window ran, the launches.  The last device run's pixels are
compared with Pillow's.  The images are synthetic renders; photographs carry more entropy per pixel."""
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
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "jpegdec_c%d.json" % a.config)

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])


def encode(img):
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", quality=90, subsampling=2)
    return f.getvalue()


def decode(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8))


with ThreadPoolExecutor(16) as pool:
    files = list(pool.map(encode, s.images))
raw_bytes = sum(int(img.size) for img in s.images)
print("scene + %d files: %.1f s, %d pixel bytes, %d file bytes" % (len(files), time.perf_counter() - t0, raw_bytes, sum(map(len, files))), flush=True)

c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
host, device = [], []
for r in range(a.runs + 1):                    # run 0 is the warm-up: buffers, code objects, the pinned ring
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        pixels = list(pool.map(decode, files))
    t1 = time.perf_counter()
    c.set_views(s.cams, pixels)
    t2 = time.perf_counter()
    st = c.set_views_jpeg(s.cams, files)
    t3 = time.perf_counter()
    if r:
        host.append({"pillow_16_threads_ms": 1e3 * (t1 - t), "set_views_ms": 1e3 * (t2 - t1)})
        st["wall_ms"] = 1e3 * (t3 - t2)
        device.append(st)
# the decoded pixels of the last run against Pillow's
got, _ = c.decode_jpegs(files[:8])
equal = all(np.array_equal(x, y) for x, y in zip(got, pixels[:8]))
x = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
y.copy_(x); torch.cuda.synchronize()
copies = []
for _ in range(a.runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
    copies.append(float(e0.elapsed_time(e1)))
c.close()

med = lambda rows, k: float(np.median([r[k] for r in rows]))
last = device[-1]
res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "views": s.n_views, "runs": a.runs,
       "files": "Pillow JPEG, quality 90, 4:2:0, no restart markers; synthetic renders (photographs carry more entropy per pixel)",
       "host_route": {"pillow_16_threads_ms": med(host, "pillow_16_threads_ms"), "set_views_ms": med(host, "set_views_ms"), "bytes_uploaded": raw_bytes,
                      "runs": host},
       "device_route": dict({k: med(device, k) for k in M.viewsel.JPEGDEC_MS + ("wall_ms",)}, bytes_uploaded=last["entropy_bytes"],
                            wall_ms_runs=[d["wall_ms"] for d in device], **{k: last[k] for k in M.viewsel.JPEGDEC_COUNTS}),
       "device_copy_of_the_pixels_ms": float(np.median(copies)),
       "sync": {"exact_after_pass1_share": last["subseq_exact_after_pass1"] / max(last["subsequences"], 1), "sync_rounds_max": last["sync_rounds_max"],
                "sync_launches": last["sync_launches"], "subsequences": last["subsequences"], "windows": last["windows"]},
       "first_8_views_equal_pillow": bool(equal),
       "note": "legs alternate in one process; medians of the timed runs after one warm-up.  host clock around each part; ms_* are device times from events on the "
               "context's stream.  The host route's time is the yardstick of the parent commit, not compared against a bound"}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
print("wrote", out_path)
