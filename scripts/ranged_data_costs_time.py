"""What walking the data costs in face ranges costs (option "dc_range_pairs", csrc/k_dc.hip dc_ranged) at a BASELINE config:
   ranged_data_costs_time.py --config 3 [--ranges 1,2,4,8,16] [--runs 3] [--out profiles/ranged_c3.json]
For every number of ranges n: B = n_views x ceil(faces / n), one fresh context, a warm-up pass, then `runs` passes timed with the
context's own device events (option "profile": milliseconds per data-cost stage, median over the runs), the `rays` ratio against the
unranged pass (one extra, untimed pass with the counters on), and the device memory the context holds after the passes -- its buffers
only grow, so that is its peak (hipMemGetInfo around the context; the caller's resident images are not part of it).  What the rows are compared
with is the FIRST row of the same run: option 0, the unranged path.  n = 1 is one range through the ranged code (kept and appended)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--ranges", default="1,2,4,8,16")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out_path = a.out or os.path.join(ROOT, "profiles", "ranged_c%d.json" % a.config)

s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
F, V = s.n_faces, s.n_views
dev = torch.device("cuda:0")
verts, faces, normals = (torch.from_numpy(x).to(dev) for x in (s.verts, s.faces.view(np.int32), s.normals))
images = [torch.from_numpy(im).to(dev) for im in s.images]
torch.cuda.synchronize()
print("scene: %d faces x %d views" % (F, V), flush=True)


def held():
    free, total = torch.cuda.mem_get_info(0)
    return total - free


rows, ref_table, ref_rays = [], None, None
for n in [0] + [int(x) for x in a.ranges.split(",")]:
    B = 0 if n == 0 else V * -(-F // n)
    before = held()
    c = M.Context(0)
    c.set_option("dc_range_pairs", B)
    c.set_mesh(verts, faces, normals); c.set_views(s.cams, images)
    c.data_costs(M.Settings())                                   # warm-up: buffers, code objects
    c.set_option("profile", 1); c.get_profile()
    runs = []
    for _ in range(a.runs):
        st = c.data_costs(M.Settings())
        runs.append({k: v[0] for k, v in c.get_profile().items() if k.startswith("dc_")})
    c.set_option("profile", 0)
    n_ranges, per = c.dc_ranges()
    peak = held() - before
    c.set_option("stats", 1)
    st = c.data_costs(M.Settings())
    tab = c.costs_download()
    c.close()
    if ref_table is None:
        ref_table, ref_rays = tab, st["rays"]
    equal = bool(np.array_equal(tab.col_ptr, ref_table.col_ptr) and np.array_equal(tab.view_id, ref_table.view_id)
                 and np.array_equal(tab.cost.view(np.uint32), ref_table.cost.view(np.uint32)))
    stages = sorted(set().union(*[r.keys() for r in runs]))
    med = {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in stages}
    row = {"dc_range_pairs": B, "ranges": n_ranges, "range_faces": per, "ms_stage_median": med, "ms_total_median": float(np.median([sum(r.values()) for r in runs])),
           "ms_total_runs": [sum(r.values()) for r in runs], "rays": st["rays"], "rays_ratio": st["rays"] / max(ref_rays, 1), "nnz": st["nnz"],
           "context_device_bytes": int(peak), "table_equals_unranged": equal}
    rows.append(row)
    print(json.dumps({k: row[k] for k in ("ranges", "range_faces", "ms_total_median", "rays_ratio", "context_device_bytes", "table_equals_unranged")}), flush=True)

res = {"config": a.config, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": F, "views": V, "runs": a.runs,
       "rows": rows,
       "note": "row 0 is the unranged path (option 0) of the same run on the same device: what the others are compared with.  Milliseconds are sums of "
               "the context's device-event spans per stage (dc_order, dc_bvh_build, dc_prep run once per pass; dc_prep on a second stream beside "
               "the first two, so the sum of the stages is above the elapsed time of a pass by what overlaps); dc_append = costs + rebased append of a "
               "ranged pass.  context_device_bytes: device memory taken between creating the context and its last pass (mesh copy, prepared views, "
               "work buffers, kept arrays, table), the caller's resident images not included."}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
