"""Row f11 restated in numpy (DESIGN.md section 4 "Model output" item 8): the BIN parts and the JSON (as a dict) of the binary glTF that
Context.build_glb gives for (verts, mesh_faces, atlases, normals), with np.unique on the (coordinate, vertex) keys -- and parse_glb, a strict
reader of such a file.  Test infrastructure only."""
import json
import struct

import numpy as np

PNG_SIG = b"\x89PNG\r\n\x1a\n"
MAGIC, JSON_CHUNK, BIN_CHUNK = 0x46546C67, 0x4E4F534A, 0x004E4942


def order_image(x):
    """the order-preserving uint32 image of float32 values: -0 < +0, and the order does not depend on how floats compare"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def bounds(pos):
    """(min, max) of an (n, 3) float32 array per column, by order_image: two (3,) float32 arrays"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    im = order_image(pos)
    return (np.array([pos[im[:, k].argmin(), k] for k in range(3)], np.float32), np.array([pos[im[:, k].argmax(), k] for k in range(3)], np.float32))


def corners(mesh_faces, atlases):
    """(v, g, atlas) of every corner c = 3 e + k in list order"""
    mf = np.ascontiguousarray(mesh_faces, np.uint32).reshape(-1, 3)
    face_ptr = np.asarray(atlases["face_ptr"], np.int64); tc_ptr = np.asarray(atlases["tc_ptr"], np.int64)
    faces = np.asarray(atlases["faces"], np.int64).reshape(-1); ids = np.asarray(atlases["texcoord_ids"], np.int64).reshape(-1, 3)
    atlas = np.repeat(np.arange(len(face_ptr) - 1), np.diff(face_ptr))
    v = mf[faces].astype(np.int64).reshape(-1)
    g = (tc_ptr[atlas][:, None] + ids).reshape(-1)
    return v, g, np.repeat(atlas, 3)


def restate(verts, mesh_faces, atlases, normals=None, pngs=None):
    """dict(bin=bytes of the BIN chunk's data (padded), json=dict, vertices=NP, first=(A + 1,), nonfinite=count): item 8 on numpy arrays.
    pngs: the PNG file of every atlas (a list of bytes) or None for a text-only set."""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    merged = np.ascontiguousarray(atlases["texcoords_merged"], np.float32).reshape(-1, 2)
    normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    face_ptr = np.asarray(atlases["face_ptr"], np.int64); tc_ptr = np.asarray(atlases["tc_ptr"], np.int64)
    A = len(face_ptr) - 1
    v, g, atlas = corners(mesh_faces, atlases)
    uniq, inverse = np.unique((g.astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64), return_inverse=True)   # ascending g, then v
    pg, pv = (uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64)
    NP = len(uniq)
    first = np.searchsorted(pg, tc_ptr, "left")                     # atlas a's pairs are [first[a], first[a + 1])
    index = (inverse.reshape(-1) - first[atlas]).astype("<u4") if len(v) else np.zeros(0, "<u4")
    pos, tex = verts[pv], merged[pg]
    parts = [pos.tobytes(), tex.tobytes()] + ([normals[pv].tobytes()] if normals is not None else []) + [index.tobytes()]
    at = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    nonfinite = int((~np.isfinite(pos)).sum()) + (int((~np.isfinite(normals[pv])).sum()) if normals is not None else 0)
    has = [a for a in range(A) if face_ptr[a + 1] > face_ptr[a]]
    nrm = normals is not None
    per, idx_view = (4, 3) if nrm else (3, 2)
    j = {"asset": {"version": "2.0", "generator": "mvs-texturing_amd"}, "scene": 0}
    views = []
    if has:
        j["scenes"] = [{"nodes": [0]}]; j["nodes"] = [{"mesh": 0}]
        prims, acc = [], []
        for q, a in enumerate(has):
            attr = {"POSITION": per * q, "TEXCOORD_0": per * q + 1}
            if nrm:
                attr["NORMAL"] = per * q + 2
            prims.append({"attributes": attr, "indices": per * q + per - 1, "material": a, "mode": 4})
            f0, cnt = int(first[a]), int(first[a + 1] - first[a])
            lo, hi = bounds(pos[f0:f0 + cnt])
            acc.append({"bufferView": 0, "byteOffset": 12 * f0, "componentType": 5126, "count": cnt, "type": "VEC3",
                        "min": [float(x) for x in lo], "max": [float(x) for x in hi]})
            acc.append({"bufferView": 1, "byteOffset": 8 * f0, "componentType": 5126, "count": cnt, "type": "VEC2"})
            if nrm:
                acc.append({"bufferView": 2, "byteOffset": 12 * f0, "componentType": 5126, "count": cnt, "type": "VEC3"})
            acc.append({"bufferView": idx_view, "byteOffset": 12 * int(face_ptr[a]), "componentType": 5125, "count": 3 * int(face_ptr[a + 1] - face_ptr[a]), "type": "SCALAR"})
        j["meshes"] = [{"primitives": prims}]; j["accessors"] = acc
        stride = [12, 8, 12] if nrm else [12, 8]
        for i, st in enumerate(stride):
            views.append({"buffer": 0, "byteOffset": int(at[i]), "byteLength": int(at[i + 1] - at[i]), "byteStride": st, "target": 34962})
        views.append({"buffer": 0, "byteOffset": int(at[idx_view]), "byteLength": int(at[idx_view + 1] - at[idx_view]), "target": 34963})
    else:
        j["scenes"] = [{}]
    data = b"".join(parts) if has else b""
    end = len(data)
    if A:
        j["materials"] = [{"name": "material%04d" % a, "pbrMetallicRoughness": dict(({"baseColorTexture": {"index": a}} if pngs is not None else {}), metallicFactor=0, roughnessFactor=1)}
                          for a in range(A)]
    if pngs is not None and A:
        assert len(pngs) == A
        v0 = len(views)
        j["textures"] = [{"sampler": 0, "source": a} for a in range(A)]
        j["images"] = [{"bufferView": v0 + a, "mimeType": "image/png"} for a in range(A)]
        j["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
        for p in pngs:
            views.append({"buffer": 0, "byteOffset": len(data), "byteLength": len(p)})
            end = len(data) + len(p)
            data += p + b"\0" * (-len(p) % 4)
    if data:
        j["bufferViews"] = views; j["buffers"] = [{"byteLength": end}]
    return dict(bin=data, json=j, vertices=NP, first=first, nonfinite=nonfinite)


def assemble(j, data):
    """the .glb of a JSON dict and the BIN chunk's data (no BIN chunk for empty data)"""
    text = json.dumps(j, separators=(",", ":")).encode()
    text += b" " * (-len(text) % 4)
    data = data + b"\0" * (-len(data) % 4)
    body = struct.pack("<II", len(text), JSON_CHUNK) + text + (struct.pack("<II", len(data), BIN_CHUNK) + data if data else b"")
    return struct.pack("<III", MAGIC, 2, 12 + len(body)) + body


_COMPONENTS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3}


def parse_glb(data):
    """Checks a .glb of row f11's kind and returns dict(json, bin, primitives=[{material, POSITION (n, 3), TEXCOORD_0 (n, 2), NORMAL (n, 3)
    or absent, indices (m,)}], images=[bytes]).  Asserts: the 12-byte header and the chunk headers, lengths, 4-byte padding with space and
    zero fill, every buffer view inside the buffer, every accessor inside its view, every count >= 1, every index below its primitive's
    vertex count and never 0xFFFFFFFF, min / max equal to the data's own, material / texture / image indices in range, the PNG signature."""
    assert len(data) >= 20 and len(data) % 4 == 0, "file length"
    magic, version, total = struct.unpack_from("<III", data, 0)
    assert magic == MAGIC and version == 2, "header"
    assert total == len(data), "length field %d, file %d" % (total, len(data))
    n_json, t_json = struct.unpack_from("<II", data, 12)
    assert t_json == JSON_CHUNK and n_json % 4 == 0 and 20 + n_json <= len(data), "JSON chunk header"
    text = data[20:20 + n_json]
    body = text.rstrip(b" ")
    assert body.endswith(b"}") and len(text) - len(body) < 4, "JSON padding"
    j = json.loads(body.decode("ascii"))
    at = 20 + n_json
    blob = b""
    if at < len(data):
        assert at + 8 <= len(data), "BIN chunk header"
        n_bin, t_bin = struct.unpack_from("<II", data, at)
        assert t_bin == BIN_CHUNK and n_bin % 4 == 0 and n_bin >= 1 and at + 8 + n_bin == len(data), "BIN chunk header"
        blob = data[at + 8:]
    buffers = j.get("buffers", [])
    assert len(buffers) == (1 if blob else 0), "buffers"
    if blob:
        used = buffers[0]["byteLength"]
        assert 1 <= used <= len(blob) < used + 4 and not any(blob[used:]), "BIN padding"
    assert j["asset"]["version"] == "2.0" and j["scene"] == 0 and len(j["scenes"]) == 1
    views = j.get("bufferViews", [])
    for v in views:
        assert v["buffer"] == 0 and v["byteOffset"] % 4 == 0 and v["byteLength"] >= 1 and v["byteOffset"] + v["byteLength"] <= buffers[0]["byteLength"], "buffer view outside the buffer"
    accessors = j.get("accessors", [])

    def read(i, dtype, kind, target):
        acc = accessors[i]
        view = views[acc["bufferView"]]
        n, k = acc["count"], _COMPONENTS[acc["type"]]
        assert acc["type"] == kind and acc["componentType"] == (5126 if dtype == "<f4" else 5125) and view.get("target") == target
        assert n >= 1, "count"
        assert view.get("byteStride", 4 * k) == 4 * k and (target == 34963) == ("byteStride" not in view)
        assert acc["byteOffset"] % 4 == 0 and acc["byteOffset"] + 4 * k * n <= view["byteLength"], "accessor outside its view"
        arr = np.frombuffer(blob, dtype, k * n, view["byteOffset"] + acc["byteOffset"])
        return acc, (arr.reshape(n, k) if k > 1 else arr)

    materials, textures, images = j.get("materials", []), j.get("textures", []), j.get("images", [])
    prims = []
    if "meshes" in j:
        assert j["scenes"] == [{"nodes": [0]}] and j["nodes"] == [{"mesh": 0}] and len(j["meshes"]) == 1 and len(j["meshes"][0]["primitives"]) >= 1
        for p in j["meshes"][0]["primitives"]:
            assert p["mode"] == 4 and 0 <= p["material"] < len(materials), "material index"
            out = {"material": p["material"]}
            acc, out["POSITION"] = read(p["attributes"]["POSITION"], "<f4", "VEC3", 34962)
            lo, hi = bounds(out["POSITION"])
            assert np.array_equal(np.array(acc["min"], np.float32).view(np.uint32), lo.view(np.uint32)), "min"
            assert np.array_equal(np.array(acc["max"], np.float32).view(np.uint32), hi.view(np.uint32)), "max"
            _, out["TEXCOORD_0"] = read(p["attributes"]["TEXCOORD_0"], "<f4", "VEC2", 34962)
            assert set(p["attributes"]) <= {"POSITION", "TEXCOORD_0", "NORMAL"}
            if "NORMAL" in p["attributes"]:
                _, out["NORMAL"] = read(p["attributes"]["NORMAL"], "<f4", "VEC3", 34962)
                assert len(out["NORMAL"]) == len(out["POSITION"])
            assert len(out["TEXCOORD_0"]) == len(out["POSITION"])
            acc, out["indices"] = read(p["indices"], "<u4", "SCALAR", 34963)
            assert acc["count"] % 3 == 0
            assert int(out["indices"].max()) < len(out["POSITION"]) and int(out["indices"].max()) != 0xFFFFFFFF, "index out of range"
            prims.append(out)
    else:
        assert j["scenes"] == [{}] and "nodes" not in j and "accessors" not in j
    for m in materials:
        pbr = m["pbrMetallicRoughness"]
        assert pbr["metallicFactor"] == 0 and pbr["roughnessFactor"] == 1
        if "baseColorTexture" in pbr:
            assert 0 <= pbr["baseColorTexture"]["index"] < len(textures), "texture index"
    for t in textures:
        assert 0 <= t["source"] < len(images) and 0 <= t["sampler"] < len(j["samplers"]), "image index"
    if "samplers" in j:
        assert j["samplers"] == [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
    pngs = []
    for im in images:
        assert im["mimeType"] == "image/png"
        v = views[im["bufferView"]]
        assert "target" not in v and "byteStride" not in v
        png = blob[v["byteOffset"]:v["byteOffset"] + v["byteLength"]]
        assert png.startswith(PNG_SIG), "PNG signature"
        pngs.append(png)
    return dict(json=j, bin=blob, primitives=prims, images=pngs)


def expand(prim):
    """the corners of a parsed primitive: (positions (m, 3), uvs (m, 2), normals (m, 3) or None)"""
    i = prim["indices"].astype(np.int64)
    return prim["POSITION"][i], prim["TEXCOORD_0"][i], (prim["NORMAL"][i] if "NORMAL" in prim else None)


def json_equal(got, want):
    """two JSON dicts equal, min / max compared as float32 bits"""
    def norm(j):
        j = json.loads(json.dumps(j))
        for acc in j.get("accessors", []):
            for k in ("min", "max"):
                if k in acc:
                    acc[k] = [int(x) for x in np.array(acc[k], np.float32).view(np.uint32)]
        return j
    return norm(got) == norm(want)
