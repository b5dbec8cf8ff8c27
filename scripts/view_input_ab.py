"""A/B of library builds over the view input alone, on ONE box in one call: the legs of undistort_time.py (b: set_views(lens=), d:
set_views_jpeg(lens=)), view_masks_time.py (set_view_masks plain and under a lens) and jpeg_decode_time.py (set_views_jpeg), wall clock and
device time, at a BASELINE config.  The scene, its JPEG files and its masks are made once; every variant runs in a forked child (own HIP
context, the variant's library only: the building-blocks library is not loaded), the variants alternate `--rounds` times.  A child runs
every leg `--runs` times after one warm-up and reports the medians, and the checksum of the table of a data-cost pass behind the last leg:
variants must agree on it.  The yardstick of a leg is the FIRST variant's own round-to-round spread (3 %, the box-to-box spread, where its
rounds coincide: closer than 0.1 % of the value).
Usage: python scripts/view_input_ab.py [--config 3] [--rounds 2] [--runs 3] [--out profiles/view_input_plumbing_ab.json] parent=path/to/lib.so new=path/to/lib.so"""
import argparse, io, json, multiprocessing as mp, os, statistics, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import mvs_texturing_amd as M


def child(lib, scene, files, masks, lens, runs, q):
    M.viewsel._LIB_PATH = os.path.abspath(lib)
    M.viewsel._BLOCKS_PATH = os.path.join(os.path.dirname(M.viewsel._LIB_PATH), "no_blocks_library_in_an_ab_child")
    c = M.Context(0)
    c.set_mesh(scene.verts, scene.faces, scene.normals)
    dec = M.viewsel.JPEGDEC_MS

    def leg(call, device):
        rows = []
        for k in range(runs + 1):                       # run 0 is the warm-up: buffers, code objects, the pinned ring
            t = time.perf_counter()
            st = call()
            wall = (time.perf_counter() - t) * 1e3
            if k:
                rows.append(dict({"wall_ms": wall}, **device(st)))
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    out = {}
    out["b_set_views_lens"] = leg(lambda: c.set_views(scene.cams, scene.images, lens=lens), lambda st: {"ms_upload": st["ms_upload"], "ms_undistort": st["ms_undistort"]})
    out["jpeg_set_views_jpeg"] = leg(lambda: c.set_views_jpeg(scene.cams, files), lambda st: {"ms_device_stages": sum(st[k] for k in dec)})
    out["masks_plain"] = leg(lambda: c.set_view_masks(masks), lambda st: {"ms_upload": st["ms_upload"], "ms_pack": st["ms_pack"]})
    out["d_set_views_jpeg_lens"] = leg(lambda: c.set_views_jpeg(scene.cams, files, lens=lens),
                                       lambda st: {"ms_device_stages": sum(st[k] for k in dec), "ms_undistort": st["lens"]["ms_undistort"]})
    out["masks_lens"] = leg(lambda: c.set_view_masks(masks, lens=lens), lambda st: {"ms_upload": st["ms_upload"], "ms_undistort": st["ms_undistort"]})
    st = c.data_costs(M.Settings())                     # undistorted JPEG views under undistorted masks: every route is in this table
    dc = c.costs_download()
    out["crc"] = zlib.crc32(dc.cost.tobytes(), zlib.crc32(dc.view_id.tobytes(), zlib.crc32(dc.col_ptr.tobytes())))
    out["nnz"] = int(st["nnz"])
    c.close()
    q.put(out)


def encode(img):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", quality=90, subsampling=2)
    return f.getvalue()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(); ap.add_argument("--config", type=int, default=3); ap.add_argument("--rounds", type=int, default=2); ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_input_plumbing_ab.json")); ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    scene = M.synth.make_scene(**M.synth.CONFIGS[a.config])
    V = scene.n_views
    h, w = scene.images[0].shape[:2]
    with ThreadPoolExecutor(16) as pool:
        files = list(pool.map(encode, scene.images))
    yy, xx = np.mgrid[0:h, 0:w]
    masks = [np.ascontiguousarray(np.where((xx - (w / 2 + (j % 7 - 3) * 11)) ** 2 + (yy - (h / 2 + (j % 5 - 2) * 9)) ** 2 <= 0.1 * w * h / np.pi, 0, 255).astype(np.uint8)) for j in range(V)]
    lens = np.array([(float(scene.cams["K"][j][0]) / max(w, h), -0.2, 0.05) for j in range(V)], np.float32)
    print("scene, %d files, %d masks ready" % (len(files), len(masks)), flush=True)
    ctx = mp.get_context("fork")
    names = [spec.partition("=")[0] for spec in a.libs]
    res = {n: [] for n in names}
    order = []
    for r in range(a.rounds):
        for spec in (a.libs if r % 2 == 0 else a.libs[::-1]):      # parent new new parent ...
            name, _, path = spec.partition("=")
            q = ctx.Queue(); p = ctx.Process(target=child, args=(path, scene, files, masks, lens, a.runs, q)); p.start()
            try:
                out = q.get(timeout=400)                # a child that died never answers: no waiting for ever on a GPU box
            except Exception:  # noqa: BLE001
                p.kill(); p.join(); raise SystemExit("variant %s: the child did not answer (exit code %s)" % (name, p.exitcode))
            p.join()
            res[name].append(out); order.append("%s_%d" % (name, r + 1))
            print(order[-1], json.dumps(out), flush=True)
    base = names[0]
    legs = {}
    for leg in [k for k in res[base][0] if k not in ("crc", "nnz")]:
        for key in res[base][0][leg]:
            ref = [x[leg][key] for x in res[base]]
            lo, hi = min(ref), max(ref)
            tol = 0.03 * hi if hi - lo < 1e-3 * max(hi, 1e-9) else 0.0          # the rounds coincide: the box-to-box spread instead
            row = {base: ref, base + "_spread": hi - lo}
            for n in names[1:]:
                v = [x[leg][key] for x in res[n]]
                m = statistics.median(v)
                row[n] = v; row[n + "_median"] = m
                row[n + "_verdict"] = "inside" if lo - tol <= m <= hi + tol else ("below: faster" if m < lo else "ABOVE")
            legs["%s.%s" % (leg, key)] = row
    doc = {"command": "scripts/view_input_ab.py --config %d --rounds %d --runs %d %s" % (a.config, a.rounds, a.runs, " ".join(names)), "order": order,
           "yardstick": "a leg's value per round is the median of %d runs after a warm-up; `inside`: the variant's median over its rounds lies within the round-to-round "
                        "spread of `%s` in this same call (3 %% where its rounds coincide: closer than 0.1 %% of the value)" % (a.runs, base),
           "same_table": len({x["crc"] for n in names for x in res[n]}) == 1, "table_crc": "%08x" % res[base][0]["crc"], "nnz": res[base][0]["nnz"], "legs": legs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    for k, row in legs.items():
        print(k, {x: (round(y, 3) if isinstance(y, float) else y) for x, y in row.items()})
    print("same table:", doc["same_table"], "wrote", a.out)
