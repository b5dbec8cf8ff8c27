"""Row f8 (texture atlases) at a BASELINE config, with labels from the library's own view selection and the patches of its rows f5 - f7,
which stay on the device:
   texture_atlases_time.py --config 3 [--runs 3] [--out profiles/atlas_c3.json] [--no-model] [--lib other/libmvs_viewsel.so --packer device] [--tone-mapping gamma]
Records the time per phase (mvs_atlas_stats, median of the timed runs after one warm-up: ms_pack is HOST time -- ordering, packing, the
per-patch tables and their uploads --, ms_compose / ms_pad / ms_texcoords are device time from events), the counters, the
bytes the composition moves (12 B of colour and 1 B of validity read, 3 B of colour, 1 B of mask and at most 1 B of level written per
patch pixel, plus 5 B cleared per atlas pixel) and the rate that makes beside a device-to-device copy of the same number of bytes, and
the single-thread time of the CPU model (tests/tools/atlas_model.cpp) -- its packing alone and the whole stage -- on the same input
with a bit-for-bit comparison of every output array and every counter.  --lib runs another build of the library (the
one-workgroup device packer of profiles/atlas_device_packer.patch: profiles/EXPERIMENTS.md "Row f8: the packer"); --packer names which packer
that build has, for the record.  When profiles/atlas_c<config>_device_packer.json exists, its packing time is copied beside this run's.
--tone-mapping gamma runs rows f5, f6 and f8 in that mode (the CPU model states `none` only: no comparison then; the default output becomes
profiles/atlas_c<config>_gamma.json).  scripts/tone_mapping_time.py measures the two modes side by side."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "tools")]
import numpy as np  # noqa: E402

import mvs_texturing_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--no-model", action="store_true")
ap.add_argument("--lib", default=None, help="another build of libmvs_viewsel.so (experiments)")
ap.add_argument("--packer", default="host", choices=["host", "device"], help="the packer the library under test has (host: the committed code)")
ap.add_argument("--tone-mapping", default="none", choices=["none", "gamma"])
a = ap.parse_args()
TONE = M.viewsel.TONE_MAPPINGS[a.tone_mapping]
if TONE:
    a.no_model = True
if a.lib:
    M.viewsel._LIB_PATH = os.path.abspath(a.lib)
out_path = a.out or os.path.join(ROOT, "profiles", "atlas_c%d%s.json" % (a.config, "_gamma" if TONE else ""))

t0 = time.perf_counter()
s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
c = M.Context(0)
c.set_mesh(s.verts, s.faces, s.normals)
c.set_views(s.cams, s.images)
c.data_costs(M.Settings())
labels, ms = c.view_selection(s.adj_ptr, s.adj)
gsl, gst = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(tone_mapping=TONE), on_device=True)
dev, pst = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], M.default_patch_params(tone_mapping=TONE), on_device=True)
lsl, lst = c.local_seam_leveling(s.adj_ptr, s.adj, labels, dev, on_device=True)
dev = dict(dev); dev.update(image=lsl["image"], validity=lsl["validity"])
print("scene + labels + rows f5 - f7: %.1f s, %d faces, %d views, %d patches, %d pixels" % (time.perf_counter() - t0, s.n_faces, s.n_views, pst["patches"], pst["pixels"]), flush=True)

AP = M.default_atlas_params(tone_mapping=TONE)
c.texture_atlases(dev, AP, on_device=True)         # warm-up: buffers, code objects
runs = []
for _ in range(a.runs):
    t = time.perf_counter()
    got, st = c.texture_atlases(dev, AP, on_device=True)
    st["wall_ms"] = 1e3 * (time.perf_counter() - t)
    runs.append(st)
phases = ("ms_pack", "ms_compose", "ms_pad", "ms_texcoords", "ms_total", "wall_ms")
med = {k: float(np.median([r[k] for r in runs])) for k in phases}
last = runs[-1]
compose_bytes = 17 * pst["pixels"] + 5 * last["pixels"]
res = {"config": a.config, "tone_mapping": a.tone_mapping, "workload": "BASELINE config %d: %s" % (a.config, M.synth.CONFIGS[a.config]), "faces": s.n_faces, "views": s.n_views,
       "labels": "the library's view selection (sweeps %d)" % ms["sweeps"], "patches": pst["patches"], "patch_pixels": pst["pixels"],
       "listed_faces": pst["listed_faces"], "runs": a.runs, "ms_median": med, "ms_runs": [{k: r[k] for k in phases} for r in runs],
       **{k: last[k] for k in M.viewsel.ATLAS_COUNTS},
       "compose": {"bytes": compose_bytes, "gb_per_s": compose_bytes / (med["ms_compose"] * 1e-3) / 1e9 if med["ms_compose"] > 0 else None},
       "packer": a.packer, "library": os.path.relpath(M.viewsel._LIB_PATH, ROOT),
       "note": "ms_pack = HOST clock: read-back of the frames excluded, ordering the patches, the packer (" + ("the one-workgroup device kernel of profiles/atlas_device_packer.patch with its upload, launch and read-back" if a.packer == "device" else "host code over vectors") + "), "
               "the per-patch tables and their uploads; the other phases are device time from events on the context's stream (compose = clearing image / mask / "
               "levels, quantise and scatter; pad = size / 128 + 1 sweeps; texcoords = coordinates, two radix sorts, heads, ranks, ids); ms_total = their sum; "
               "wall_ms = host clock around the call; inputs and outputs stay on the device"}
try:
    import torch
    n = int(compose_bytes) // 2                      # a copy reads n and writes n: the same traffic
    x = torch.empty(n, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
    y.copy_(x); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize()
    res["compose"]["device_copy_same_bytes_ms"] = float(e0.elapsed_time(e1))
    res["compose"]["device_copy_gb_per_s"] = compose_bytes / (res["compose"]["device_copy_same_bytes_ms"] * 1e-3) / 1e9
    del x, y
except ImportError:
    pass
print(json.dumps({k: res[k] for k in ("ms_median", "atlases", "pixels", "padded_pixels", "free_rects_peak", "merged_texcoords", "compose")}), flush=True)

if not a.no_model:
    import atlas_model as AM
    import torch

    def dev_host(d, dtype):
        dt = np.dtype(dtype); n = d.shape[0]
        if n == 0:
            return np.zeros(0, dt)

        class _Dev:
            __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (d.data_ptr(), False), "version": 2}
        return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt)
    host = {k: dev_host(got[k], dt) for k, dt in AM.ARRAYS.items()}
    pa = {k: dev_host(dev[k], dt) for k, dt in AM.PATCH_ARRAYS.items()}
    AM.build()
    stm, _, _, _, pack_ms = AM.run(pa, pack_only=True)
    res["model_pack_single_thread_ms"] = pack_ms[0]
    t = time.perf_counter()
    stm, want, wst, cnt, mms = AM.run(pa)
    res["model_single_thread_s"] = time.perf_counter() - t
    res["model_counters"] = cnt
    ok = stm == 0 and all(last[k] == wst[k] for k in AM.STATS)
    for k in AM.ARRAYS:
        ok = ok and host[k].size == want[k].size and np.array_equal(host[k].view(np.uint8).ravel(), np.ascontiguousarray(want[k]).view(np.uint8).ravel())
    res["model_equal"] = bool(ok)
    res["pack"] = {"packer": a.packer, "library_ms_pack": med["ms_pack"], "model_pack_single_thread_ms": pack_ms[0]}
    rec = os.path.join(ROOT, "profiles", "atlas_c%d_device_packer.json" % a.config)
    if a.packer == "host" and os.path.exists(rec):
        with open(rec) as f:
            d = json.load(f)
        res["pack"]["device_packer_ms_pack"] = d["ms_median"]["ms_pack"]
        res["pack"]["device_packer_model_pack_single_thread_ms"] = d.get("model_pack_single_thread_ms")
        res["pack"]["device_packer_is_faster_than_model"] = bool(d["ms_median"]["ms_pack"] < d.get("model_pack_single_thread_ms", 0.0))
        res["pack"]["device_packer_record"] = os.path.relpath(rec, ROOT)
    print("model: pack %.2f ms (library, %s packer: %.2f ms), whole stage %.1f s single thread, equal: %s" % (pack_ms[0], a.packer, med["ms_pack"], res["model_single_thread_s"], res["model_equal"]), flush=True)
c.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
