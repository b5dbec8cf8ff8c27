"""Tone mapping `gamma` beside `none` at a BASELINE config, and `none` beside another checkout of the library (the parent commit), on one
GPU box in one run:
   tone_mapping_time.py --config 3 [--rounds 3] [--parent DIR] [--out profiles/tone_c3.json]
Every measurement runs in a process of its own (a fresh HIP context), this checkout and the one under DIR (a directory that holds a built
`mvs-texturing_amd` package) alternating `--rounds` times.  A process builds the scene, takes labels from the library's own view selection,
runs rows f5 - f7 in the mode and records the median of three timed calls after a warm-up of row f6's ms_resolve and row f8's ms_compose
(device events, mvs_patch_stats / mvs_atlas_stats).  This checkout measures both modes in one process, and beside them a plain device
copy of the bytes resolve and compose move (as texture_patches_time.py / texture_atlases_time.py count them) and Context.gamma_correct on
the patch image (device time of the kernel, option "profile"; 8 bytes per value).  The record holds every round, the medians, and the
run-to-run spread (max - min over the rounds) of `none` on either checkout: what `none` may differ by between the two."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_package(directory):
    """the package `mvs-texturing_amd` of a checkout (mvs_texturing_amd.py's alias, for any directory)"""
    d = os.path.join(os.path.abspath(directory), "mvs-texturing_amd")
    spec = importlib.util.spec_from_file_location("mvs_texturing_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mvs_texturing_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def copy_ms(nbytes, reps=5):
    """ms of a device-to-device copy that moves nbytes in total (half read, half written)"""
    import numpy as np
    import torch
    n = max(int(nbytes) // 2, 1)
    src = torch.empty(n, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    src.zero_(); dst.copy_(src); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def child(a):
    import numpy as np
    M = load_package(a.package)
    s = M.synth.make_scene(**M.synth.CONFIGS[a.config])
    c = M.Context(0)
    c.set_mesh(s.verts, s.faces, s.normals)
    c.set_views(s.cams, s.images)
    c.data_costs(M.Settings())
    labels, _ = c.view_selection(s.adj_ptr, s.adj)
    out = {"package": os.path.relpath(os.path.abspath(a.package), ROOT), "modes": {}}
    for mode in a.modes.split(","):
        tone = {} if mode == "none" else dict(tone_mapping=1)           # (a checkout without the field runs `none` only)
        gsl, _ = c.global_seam_leveling(s.adj_ptr, s.adj, labels, M.default_gsl_params(**tone), on_device=True)
        pp, ap = M.default_patch_params(**tone), M.default_atlas_params(**tone)
        c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], pp, on_device=True)        # warm-up: buffers, code objects
        resolve = []
        for _ in range(3):
            dev, pst = c.texture_patches(s.adj_ptr, s.adj, labels, gsl["corner_adjust"], pp, on_device=True)
            resolve.append(pst["ms_resolve"])
        lsl, _ = c.local_seam_leveling(s.adj_ptr, s.adj, labels, dev, on_device=True)
        dev = dict(dev); dev.update(image=lsl["image"], validity=lsl["validity"])
        c.texture_atlases(dev, ap, on_device=True)
        compose = []
        for _ in range(3):
            _, ast = c.texture_atlases(dev, ap, on_device=True)
            compose.append(ast["ms_compose"])
        out["modes"][mode] = {"ms_resolve": float(np.median(resolve)), "ms_compose": float(np.median(compose)), "ms_resolve_runs": resolve, "ms_compose_runs": compose}
        out["patch_pixels"], out["atlas_pixels"] = pst["pixels"], ast["pixels"]
    if a.extras:
        import torch
        NP, NA = out["patch_pixels"], out["atlas_pixels"]
        out["resolve_bytes"], out["compose_bytes"] = (8 + 3 + 12 + 2) * NP, 17 * NP + 5 * NA
        out["copy_resolve_bytes_ms"], out["copy_compose_bytes_ms"] = copy_ms(out["resolve_bytes"]), copy_ms(out["compose_bytes"])
        values = torch.rand(3 * NP, dtype=torch.float32, device="cuda")  # the size of the patch image; the time does not depend on the values' bits
        c.set_option("profile", 1)
        c.gamma_correct(values, 1.0 / 2.2); c.get_profile()
        ms = []
        for _ in range(3):
            c.gamma_correct(values, 1.0 / 2.2)
            ms.append(c.get_profile()["gamma_correct"][0])
        out["gamma_correct"] = {"values": 3 * NP, "ms": float(np.median(ms)), "gb_per_s": 8 * 3 * NP / (float(np.median(ms)) * 1e-3) / 1e9}
    c.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a directory with a built mvs-texturing_amd package of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true"); ap.add_argument("--package", default=ROOT); ap.add_argument("--modes", default="none")
    ap.add_argument("--extras", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    rounds = []
    for r in range(a.rounds):
        for name, package, modes in (("parent", a.parent, "none"), ("this", ROOT, "none,gamma")):
            if package is None:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", str(a.config), "--package", package, "--modes", modes]
            if name == "this" and r == a.rounds - 1:
                cmd.append("--extras")
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:                                         # nothing more is started on the device after a failure
                raise SystemExit("%s, round %d: exit code %d\n%s" % (name, r, p.returncode, (p.stdout + p.stderr)[-2000:]))
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            res.update(checkout=name, round=r)
            rounds.append(res)
            print(name, r, json.dumps(res["modes"]), flush=True)
    pick = lambda name, mode, key: [x["modes"][mode][key] for x in rounds if x["checkout"] == name and mode in x["modes"]]
    summary = {}
    for name, mode in (("parent", "none"), ("this", "none"), ("this", "gamma")):
        for key in ("ms_resolve", "ms_compose"):
            v = pick(name, mode, key)
            if v:
                summary["%s/%s/%s" % (name, mode, key)] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": max(v) - min(v), "rounds": v}
    last = [x for x in rounds if "gamma_correct" in x][-1]
    res = {"config": a.config, "rounds": a.rounds, "patch_pixels": last["patch_pixels"], "atlas_pixels": last["atlas_pixels"], "summary": summary,
           "resolve_bytes": last["resolve_bytes"], "compose_bytes": last["compose_bytes"], "copy_resolve_bytes_ms": last["copy_resolve_bytes_ms"],
           "copy_compose_bytes_ms": last["copy_compose_bytes_ms"], "gamma_correct": last["gamma_correct"], "all_rounds": rounds,
           "note": "one box, one run; every entry of `rounds` is the median of three timed calls after a warm-up in a process of its own, the two checkouts "
                   "alternating; spread = max - min over the rounds; device time from events (ms_resolve: row f6's resolve kernel; ms_compose: row f8's clears, "
                   "quantise and scatter); copy_*_ms: a plain device copy of the bytes the phase moves; gamma_correct: the kernel alone on 3 x patch_pixels values"}
    if a.parent:
        for key in ("ms_resolve", "ms_compose"):
            p, t = summary["parent/none/" + key], summary["this/none/" + key]
            res["none_vs_parent/" + key] = {"difference_of_medians": t["median"] - p["median"], "spread_parent": p["spread"], "spread_this": t["spread"],
                                            "within_spread": bool(abs(t["median"] - p["median"]) <= max(p["spread"], t["spread"]))}
    out_path = a.out or os.path.join(ROOT, "profiles", "tone_c%d.json" % a.config)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "all_rounds"}, indent=1))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
