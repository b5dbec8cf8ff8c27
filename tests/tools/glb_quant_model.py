"""Row f11 under glb_quantize = 1 restated in numpy (DESIGN.md section 4 "Model output" item 10, KHR_mesh_quantization): the BIN parts and
the JSON (as a dict) of the quantised binary glTF that Context.build_glb gives, on top of item 8's pairs and numbering from glb_model.py --
and parse_glb, a strict reader of such a file that leaves the container to glb_model.parse_glb.  Test infrastructure only."""
import contextlib
import json
import types

import numpy as np

import glb_model as GM

JPEG_SIG = b"\xff\xd8\xff\xe0\x00\x10JFIF\x00"
EXT = "KHR_mesh_quantization"


# ---- the arithmetic of item 10: float64 + - * / sqrt and conversions only ----

def grid(pos):
    """(lo (3,) float32, E float64, S float64) of ALL positions of a file ((n, 3) float32, n >= 1): bounds in the order of the integer
    images (-0 < +0), E the largest extent, S the step"""
    lo, hi = GM.bounds(pos)
    E = np.float64(max(np.float64(hi[j]) - np.float64(lo[j]) for j in range(3)))
    return lo, E, (np.float64(1.0) if E == 0 else E / np.float64(65535.0))


def quantise_positions(pos, lo, E):
    """(n, 3) uint16: min(65535, trunc(((x - lo) / E) * 65535 + 0.5)), all 0 for E == 0"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    if E == 0:
        return np.zeros(pos.shape, np.uint16)
    t = ((pos.astype(np.float64) - lo.astype(np.float64)[None, :]) / np.float64(E)) * np.float64(65535.0) + np.float64(0.5)
    return np.minimum(np.trunc(t), 65535.0).astype(np.uint16)


def texcoords_storable(tex):
    """bool per value: in [0, 1] (-0 is, nan is not)"""
    tex = np.asarray(tex, np.float32)
    with np.errstate(invalid="ignore"):
        return (tex >= 0) & (tex <= 1)


def quantise_texcoords(tex):
    """uint16 per value: trunc(u * 65535 + 0.5); 0 where the value cannot be stored (such a file is refused)"""
    tex = np.ascontiguousarray(tex, np.float32)
    ok = texcoords_storable(tex)
    t = np.where(ok, tex, np.float32(0)).astype(np.float64) * np.float64(65535.0) + np.float64(0.5)
    return np.trunc(t).astype(np.uint16)


def quantise_normals(nrm):
    """((n, 3) int8, zero (n,) bool): the unit normal times 127, halves away from zero; (0, 0, 0) where the length is 0"""
    n = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3).astype(np.float64)
    l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    zero = l == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (n / np.where(zero, 1.0, l)[:, None]) * np.float64(127.0)
    r = np.nan_to_num(np.minimum(np.trunc(np.abs(c) + np.float64(0.5)), 127.0))   # (a non-finite normal: such a file is refused)
    q = np.where(c < 0, -r, r).astype(np.int8)
    q[zero] = 0
    return q, zero


def index_layout(first, face_ptr):
    """(width (A,) of 2 or 4 bytes, offset (A + 1,)): 2-byte indices for an atlas of at most 65 535 vertices, every atlas from a multiple of 4"""
    first = np.asarray(first, np.int64); face_ptr = np.asarray(face_ptr, np.int64)
    width = np.where(np.diff(first) <= 65535, 2, 4)
    size = (width * 3 * np.diff(face_ptr) + 3) // 4 * 4
    return width, np.concatenate([[0], np.cumsum(size)]).astype(np.int64)


def restate(verts, mesh_faces, atlases, normals=None, images=None, mime="image/png"):
    """dict(bin, json, vertices, first, nonfinite, texcoords_out_of_range, zero_normals, index16_primitives, lo, S): item 10 on numpy arrays.
    images: the image file of every atlas (a list of bytes) or None for a text-only set."""
    base = GM.restate(verts, mesh_faces, atlases, normals, None)      # pairs, numbering, materials: item 8's
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    merged = np.ascontiguousarray(atlases["texcoords_merged"], np.float32).reshape(-1, 2)
    face_ptr = np.asarray(atlases["face_ptr"], np.int64); tc_ptr = np.asarray(atlases["tc_ptr"], np.int64)
    A = len(face_ptr) - 1
    v, g, atlas = GM.corners(mesh_faces, atlases)
    uniq, inverse = np.unique((g.astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64), return_inverse=True)
    pg, pv = (uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64)
    NP = len(uniq)
    first = np.searchsorted(pg, tc_ptr, "left")
    assert NP == base["vertices"] and np.array_equal(first, base["first"])
    has = [a for a in range(A) if face_ptr[a + 1] > face_ptr[a]]
    nrm = normals is not None
    out = dict(vertices=NP, first=first, nonfinite=base["nonfinite"], texcoords_out_of_range=0, zero_normals=0, index16_primitives=0, lo=None, S=None)
    j = {"asset": {"version": "2.0", "generator": "mvs-texturing_amd"}, "scene": 0, "extensionsUsed": [EXT], "extensionsRequired": [EXT]}
    views, data = [], b""
    if has:
        pos, tex = verts[pv], merged[pg]
        lo, E, S = grid(pos)
        qpos = quantise_positions(pos, lo, E)
        out["texcoords_out_of_range"] = int((~texcoords_storable(tex)).sum())
        part_pos = np.zeros((NP, 4), "<u2"); part_pos[:, :3] = qpos
        parts = [part_pos.tobytes(), quantise_texcoords(tex).astype("<u2").tobytes()]
        if nrm:
            qn, zero = quantise_normals(np.ascontiguousarray(normals, np.float32).reshape(-1, 3)[pv])
            part_n = np.zeros((NP, 4), np.int8); part_n[:, :3] = qn
            parts.append(part_n.tobytes())
            out["zero_normals"] = int(zero.sum())
        width, ioff = index_layout(first, face_ptr)
        local = inverse.reshape(-1) - first[atlas]
        idx = bytearray(int(ioff[-1]))
        for a in has:
            mine = local[3 * face_ptr[a]:3 * face_ptr[a + 1]].astype("<u2" if width[a] == 2 else "<u4").tobytes()
            idx[int(ioff[a]):int(ioff[a]) + len(mine)] = mine
        parts.append(bytes(idx))
        at = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        per, idx_view = (4, 3) if nrm else (3, 2)
        j["scenes"] = [{"nodes": [0]}]
        j["nodes"] = [{"mesh": 0, "translation": [float(x) for x in lo], "scale": [float(S)] * 3}]
        prims, acc = [], []
        for q, a in enumerate(has):
            attr = {"POSITION": per * q, "TEXCOORD_0": per * q + 1}
            if nrm:
                attr["NORMAL"] = per * q + 2
            prims.append({"attributes": attr, "indices": per * q + per - 1, "material": a, "mode": 4})
            f0, cnt = int(first[a]), int(first[a + 1] - first[a])
            mine = qpos[f0:f0 + cnt].astype(np.int64)
            acc.append({"bufferView": 0, "byteOffset": 8 * f0, "componentType": 5123, "count": cnt, "type": "VEC3",
                        "min": [int(x) for x in mine.min(0)], "max": [int(x) for x in mine.max(0)]})
            acc.append({"bufferView": 1, "byteOffset": 4 * f0, "componentType": 5123, "normalized": True, "count": cnt, "type": "VEC2"})
            if nrm:
                acc.append({"bufferView": 2, "byteOffset": 4 * f0, "componentType": 5120, "normalized": True, "count": cnt, "type": "VEC3"})
            acc.append({"bufferView": idx_view, "byteOffset": int(ioff[a]), "componentType": 5123 if width[a] == 2 else 5125,
                        "count": 3 * int(face_ptr[a + 1] - face_ptr[a]), "type": "SCALAR"})
            out["index16_primitives"] += int(width[a] == 2)
        j["meshes"] = [{"primitives": prims}]; j["accessors"] = acc
        for i, stride in enumerate([8, 4, 4] if nrm else [8, 4]):
            views.append({"buffer": 0, "byteOffset": int(at[i]), "byteLength": int(at[i + 1] - at[i]), "byteStride": stride, "target": 34962})
        views.append({"buffer": 0, "byteOffset": int(at[idx_view]), "byteLength": int(at[idx_view + 1] - at[idx_view]), "target": 34963})
        data = b"".join(parts)
        out.update(lo=lo, S=float(S))
    else:
        j["scenes"] = [{}]
    end = len(data)
    if "materials" in base["json"]:
        j["materials"] = [dict(m) for m in base["json"]["materials"]]
    if images is not None and A:
        assert len(images) == A
        v0 = len(views)
        for a in range(A):
            j["materials"][a]["pbrMetallicRoughness"] = dict({"baseColorTexture": {"index": a}}, metallicFactor=0, roughnessFactor=1)
        j["textures"] = [{"sampler": 0, "source": a} for a in range(A)]
        j["images"] = [{"bufferView": v0 + a, "mimeType": mime} for a in range(A)]
        j["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
        for p in images:
            views.append({"buffer": 0, "byteOffset": len(data), "byteLength": len(p)})
            end = len(data) + len(p)
            data += p + b"\0" * (-len(p) % 4)
    if data:
        j["bufferViews"] = views; j["buffers"] = [{"byteLength": end}]
    out.update(bin=data, json=j)
    return out


# ---- the reader ----

@contextlib.contextmanager
def _container_only(seen):
    """glb_model.parse_glb reads a quantised file's container, views, materials and images with its own strictness when the mesh is kept
    from it: inside this context its JSON loader hands it the file's JSON without extension, nodes, meshes and accessors (and a JPEG as
    the image kind it knows).  seen: gets the untouched JSON."""
    def loads(text):
        seen.append(json.loads(text))
        j = json.loads(text)
        for k in ("extensionsUsed", "extensionsRequired", "nodes", "meshes", "accessors"):
            j.pop(k, None)
        j["scenes"] = [{}]
        images = j.get("images", [])
        if images and all(im["mimeType"] == "image/jpeg" for im in images):
            GM.PNG_SIG = JPEG_SIG
            for im in images:
                im["mimeType"] = "image/png"
        return j
    old = GM.json, GM.PNG_SIG
    GM.json = types.SimpleNamespace(loads=loads, dumps=json.dumps)
    try:
        yield
    finally:
        GM.json, GM.PNG_SIG = old


_COMPONENT = {5120: ("i1", 1), 5123: ("<u2", 2), 5125: ("<u4", 4)}
_COUNT = {"SCALAR": 1, "VEC2": 2, "VEC3": 3}


def parse_glb(data):
    """Checks a .glb of item 10's kind and returns dict(json, bin, primitives=[{material, POSITION (n, 3) uint16, TEXCOORD_0 (n, 2) uint16,
    NORMAL (n, 3) int8 or absent, indices (m,), index_bytes 2 | 4}], images=[bytes], translation (3,) float32, scale float).
    The container is glb_model.parse_glb's business (header, chunks, padding, views inside the buffer, materials, textures, images);
    here: the extension used and required, the node's transform, every accessor's component type, normalized flag, stride and padding
    bytes, offsets at multiples of 4, min / max equal to the stored integers' own, 16-bit indices exactly where a primitive has at most
    65 535 vertices, every index below its primitive's vertex count and never the restart value."""
    seen = []
    with _container_only(seen):
        shell = GM.parse_glb(data)
    j, blob = seen[0], shell["bin"]
    assert shell["primitives"] == []
    assert j.get("extensionsUsed") == [EXT] and j.get("extensionsRequired") == [EXT], "extension"
    views, accessors = j.get("bufferViews", []), j.get("accessors", [])
    out = dict(json=j, bin=blob, primitives=[], images=shell["images"], translation=None, scale=None)
    if "meshes" not in j:
        assert j["scenes"] == [{}] and "nodes" not in j and "accessors" not in j
        return out
    assert j["scenes"] == [{"nodes": [0]}] and len(j["nodes"]) == 1 and len(j["meshes"]) == 1 and len(j["meshes"][0]["primitives"]) >= 1
    node = j["nodes"][0]
    assert set(node) == {"mesh", "translation", "scale"} and node["mesh"] == 0 and len(node["translation"]) == 3
    assert len(node["scale"]) == 3 and node["scale"][0] == node["scale"][1] == node["scale"][2] and node["scale"][0] > 0
    assert all(isinstance(x, float) for x in node["translation"] + node["scale"]), "a transform printed as an integer"
    out["translation"] = np.array(node["translation"], np.float32); out["scale"] = float(node["scale"][0])

    def read(i, component, kind, stride, normalized, target):
        acc = accessors[i]
        view = views[acc["bufferView"]]
        dtype, size = _COMPONENT[component]
        n, k = acc["count"], _COUNT[kind]
        assert acc["type"] == kind and acc["componentType"] == component and view.get("target") == target, "accessor kind"
        assert acc.get("normalized", False) is normalized and ("normalized" in acc) == normalized, "normalized"
        assert n >= 1, "count"
        assert view.get("byteStride") == stride, "byteStride"
        step = stride or size * k
        assert acc["byteOffset"] % 4 == 0 and view["byteOffset"] % 4 == 0, "a start that is no multiple of 4"
        assert acc["byteOffset"] + step * (n - 1) + size * k <= view["byteLength"], "accessor outside its view"
        start = view["byteOffset"] + acc["byteOffset"]
        rows = np.frombuffer(blob, np.uint8, step * n if stride else size * k * n, start).reshape(n, -1)
        assert not rows[:, size * k:].any(), "padding bytes inside a stride"
        arr = np.ascontiguousarray(rows[:, :size * k]).view(dtype).reshape(n, k)
        return acc, view, (arr if k > 1 else arr.reshape(-1))

    for p in j["meshes"][0]["primitives"]:
        assert p["mode"] == 4 and 0 <= p["material"] < len(j.get("materials", [])), "material index"
        assert set(p["attributes"]) <= {"POSITION", "TEXCOORD_0", "NORMAL"}
        prim = {"material": p["material"]}
        acc, _, prim["POSITION"] = read(p["attributes"]["POSITION"], 5123, "VEC3", 8, False, 34962)
        assert all(isinstance(x, int) for x in acc["min"] + acc["max"]), "min / max printed as floats"
        assert acc["min"] == prim["POSITION"].min(0).tolist(), "min"
        assert acc["max"] == prim["POSITION"].max(0).tolist(), "max"
        _, _, prim["TEXCOORD_0"] = read(p["attributes"]["TEXCOORD_0"], 5123, "VEC2", 4, True, 34962)
        assert len(prim["TEXCOORD_0"]) == len(prim["POSITION"])
        if "NORMAL" in p["attributes"]:
            _, _, prim["NORMAL"] = read(p["attributes"]["NORMAL"], 5120, "VEC3", 4, True, 34962)
            assert len(prim["NORMAL"]) == len(prim["POSITION"]) and int(prim["NORMAL"].min()) >= -127
        n = len(prim["POSITION"])
        component = 5123 if n <= 65535 else 5125
        acc, view, prim["indices"] = read(p["indices"], component, "SCALAR", None, False, 34963)
        prim["index_bytes"] = 2 if component == 5123 else 4
        assert acc["count"] % 3 == 0
        assert int(prim["indices"].max()) < n and int(prim["indices"].max()) != (0xFFFF if component == 5123 else 0xFFFFFFFF), "index out of range"
        used = view["byteOffset"] + acc["byteOffset"] + prim["index_bytes"] * acc["count"]
        assert not any(blob[used:(used + 3) // 4 * 4]), "padding behind a primitive's indices"
        out["primitives"].append(prim)
    return out


def expand(parsed, prim):
    """the corners of a parsed primitive, dequantised in float64: (positions (m, 3) = translation + q * scale, uvs (m, 2) = q / 65535,
    normals (m, 3) = max(q / 127, -1) or None)"""
    i = prim["indices"].astype(np.int64)
    pos = parsed["translation"].astype(np.float64)[None, :] + prim["POSITION"][i].astype(np.float64) * np.float64(parsed["scale"])
    uv = prim["TEXCOORD_0"][i].astype(np.float64) / 65535.0
    nrm = np.maximum(prim["NORMAL"][i].astype(np.float64) / 127.0, -1.0) if "NORMAL" in prim else None
    return pos, uv, nrm


def position_bound(x, lo, S):
    """item 10's bound on |lo + q S - x| (all float64): (0.5 + 2^-20) S + 2^-50 max(|x|, |lo|)"""
    return (0.5 + 2.0 ** -20) * S + 2.0 ** -50 * np.maximum(np.abs(x), np.abs(lo))


TEXCOORD_BOUND = 0.5 / 65535
NORMAL_BOUND = 0.5 / 127 + 2.0 ** -40


def json_equal(got, want):
    """two JSON dicts of item 10 equal: the node's translation compared as float32 bits (it is printed with 9 digits), everything else --
    the scale's float64 and the integer min / max among it -- value for value"""
    def norm(j):
        j = json.loads(json.dumps(j))
        for node in j.get("nodes", []):
            if "translation" in node:
                node["translation"] = [int(x) for x in np.array(node["translation"], np.float32).view(np.uint32)]
        return j
    return norm(got) == norm(want)
