"""View masks at a BASELINE config: every view carries a mask, a disc in the middle of the frame that covers about 10 % of it.
   view_masks_time.py --config 3 [--runs 3] [--out profiles/view_masks_c3.json]
In one process on one box, medians of the timed runs after one warm-up:
   set_view_masks on host masks: wall clock, and the library's split into upload (host time of the pinned ring), pack (device time of
     mask_pack_kernel) and undistort (device time of lens_mask_kernel) -- once with the masks used as they are, once with every mask in
     the camera's frame under a k2k4 lens;
   a device copy of the mask bytes (torch, same bytes, same box) beside the pack kernel, as its yardstick;
   the image preparation of a data-cost pass (profile span dc_prep) and the whole pass, with and without masks, alternating;
   the pairs of the table with and without masks."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "view_masks_c%d.json" % a.config)

s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
V = s.n_views
h, w = s.images[0].shape[:2]
yy, xx = np.mgrid[0:h, 0:w]
r2 = 0.1 * w * h / np.pi
masks = []
for j in range(V):      # the disc wanders a little from view to view: no two masks are the same bytes
    cx, cy = w / 2 + (j % 7 - 3) * 11, h / 2 + (j % 5 - 2) * 9
    masks.append(np.ascontiguousarray(np.where((xx - cx) ** 2 + (yy - cy) ** 2 <= r2, 0, 255).astype(np.uint8)))
mask_bytes = sum(int(m.size) for m in masks)
flen = [float(s.cams["K"][j][0]) / max(w, h) for j in range(V)]
lens = np.array([(flen[j], -0.2, 0.05) for j in range(V)], np.float32)

med = statistics.median
c = M.Context(0)
c.set_option("profile", 1)
c.set_mesh(s.verts, s.faces, s.normals)
c.set_views(s.cams, s.images)


def time_masks(lens_rows):
    runs = []
    for k in range(a.runs + 1):
        t = time.perf_counter()
        st = c.set_view_masks(masks, lens=lens_rows)
        st["wall_ms"] = (time.perf_counter() - t) * 1e3
        if k:
            runs.append(st)
    return {key: (med(x[key] for x in runs) if key.startswith("ms_") or key == "wall_ms" else runs[-1][key]) for key in runs[0]}


plain_masks = time_masks(None)
lens_masks = time_masks(lens)

# the yardstick: a device copy of the mask bytes (read once, written once; the pack kernel reads them and writes 1 / 8 of them)
src = torch.empty(mask_bytes, dtype=torch.uint8, device="cuda:0").random_(0, 2)
dst = torch.empty_like(src)
copy_ms = []
for k in range(a.runs + 1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
    if k:
        copy_ms.append(e0.elapsed_time(e1))
del src, dst


def one_pass(with_masks):
    c.set_view_masks(masks if with_masks else None)
    c.get_profile()
    t = time.perf_counter()
    st = c.data_costs(M.Settings())
    c.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    p = c.get_profile()
    return {"dc_prep_ms": p["dc_prep"][0], "data_costs_wall_ms": wall, "nnz": int(st["nnz"]), "pairs": int(st.get("pairs", 0))}


legs = {False: [], True: []}
for k in range(a.runs + 1):
    for flag in (False, True):
        r = one_pass(flag)
        if k:
            legs[flag].append(r)
prep = {name: {key: (med(x[key] for x in legs[flag]) if key.endswith("_ms") else legs[flag][-1][key]) for key in legs[flag][0]}
        for name, flag in (("without_masks", False), ("with_masks", True))}
c.close()

pack_ms = plain_masks["ms_pack"]
res = {
    "config": a.config, "views": V, "width": w, "height": h, "runs": a.runs, "mask_bytes": mask_bytes, "masked_share": float(np.mean([float((m == 0).mean()) for m in masks])),
    "set_view_masks": plain_masks, "set_view_masks_lens_k2k4": lens_masks,
    "device_copy_of_mask_bytes_ms": med(copy_ms), "device_copy_gb_s": 2 * mask_bytes / (med(copy_ms) * 1e6),
    "pack_kernel_ms": pack_ms, "pack_kernel_read_gb_s": mask_bytes / (pack_ms * 1e6) if pack_ms > 0 else None,
    "pack_over_copy": pack_ms / med(copy_ms),
    "image_prep": prep,
}
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
