"""ctypes driver of the CPU model of row f9 (obj_model.cpp; DESIGN.md section 4 "Model output"), crafted inputs for it, and a strict
line-by-line parser of the .obj grammar.  Built on first use with g++ -O2 -ffp-contract=off -fno-fast-math.  Test infrastructure only."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "obj_model.cpp")
LIB = os.path.join(HERE, "libobj_model.so")
_lib = None


def build(force=False):
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c++17", "-shared", "-o", LIB, SRC])
    return LIB


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp = C.c_void_p
        L.obj_model_run.restype = vp
        L.obj_model_run.argtypes = [C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_char_p]
        L.obj_model_floats.restype = vp; L.obj_model_floats.argtypes = [C.c_uint64, vp]
        L.obj_model_text.restype = vp; L.obj_model_text.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64)]
        L.obj_model_free.argtypes = [vp]
        _lib = L
    return _lib


def _text(L, h, which):
    n = C.c_uint64()
    p = L.obj_model_text(h, which, C.byref(n))
    return C.string_at(p, n.value)


def run(verts, mesh_faces, atlases, normals=None, name="model"):
    """(obj bytes, mtl bytes) of the mesh and the atlas-set dict (face_ptr, faces, tc_ptr, texcoords_merged, texcoord_ids)"""
    L = load()
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1); mesh_faces = np.ascontiguousarray(mesh_faces, np.uint32).reshape(-1)
    normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1)
    a = {k: np.ascontiguousarray(atlases[k], dt).reshape(-1) for k, dt in (("face_ptr", np.uint32), ("faces", np.uint32), ("tc_ptr", np.uint32),
                                                                          ("texcoords_merged", np.float32), ("texcoord_ids", np.uint32))}
    A = max(a["face_ptr"].size - 1, 0)
    ptr = lambda x: x.ctypes.data if x is not None and x.size else None
    h = L.obj_model_run(verts.size // 3, ptr(verts), ptr(mesh_faces), ptr(normals) if normals is not None else None, A, ptr(a["face_ptr"]), ptr(a["faces"]),
                        ptr(a["tc_ptr"]), ptr(a["texcoords_merged"]), ptr(a["texcoord_ids"]), name.encode())
    try:
        return _text(L, h, 0), _text(L, h, 1)
    finally:
        L.obj_model_free(h)


def format_floats(x):
    """the floats of x, one per line, as the model's stream prints them (bytes)"""
    L = load()
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    h = L.obj_model_floats(x.size, x.ctypes.data if x.size else None)
    try:
        return _text(L, h, 0)
    finally:
        L.obj_model_free(h)


EMPTY_ATLASES = dict(face_ptr=np.zeros(1, np.uint32), faces=np.zeros(0, np.uint32), tc_ptr=np.zeros(1, np.uint32), texcoords_merged=np.zeros(0, np.float32),
                     texcoord_ids=np.zeros(0, np.uint32))


# ---- the float grid of the issue ----

def float_grid(seed=20240611):
    """uint32 bit patterns: every exponent 0 .. 255 with mantissas 0, 1, 0x7FFFFF and 64 random ones, both signs; every k / 2^n with n <= 12,
    k < 4096 (the ties), both signs"""
    rng = np.random.default_rng(seed)
    man = np.concatenate([np.array([0, 1, 0x7FFFFF], np.uint32)[None, :].repeat(256, 0), rng.integers(0, 1 << 23, (256, 64), dtype=np.uint32)], 1)
    bits = (np.arange(256, dtype=np.uint32)[:, None] << np.uint32(23)) | man
    bits = np.concatenate([bits.reshape(-1), bits.reshape(-1) | np.uint32(0x80000000)])
    k = np.arange(4096, dtype=np.float32)
    ties = np.concatenate([k / np.float32(2.0 ** n) for n in range(13)])
    ties = np.concatenate([ties, -ties]).astype(np.float32)
    return np.concatenate([bits, ties.view(np.uint32)])


def snprintf_floats(bits):
    """printf("%.6f") of every bit pattern through libc (bytes, one per line); nan / -nan by sign bit"""
    libc = C.CDLL(None)
    libc.snprintf.restype = C.c_int
    buf = C.create_string_buffer(96)
    out = []
    x = np.asarray(bits, np.uint32).view(np.float32)
    for b, v in zip(np.asarray(bits, np.uint32).tolist(), x.tolist()):
        if v != v:
            out.append(b"-nan" if b >> 31 else b"nan")
        else:
            libc.snprintf(buf, C.c_size_t(96), b"%.6f", C.c_double(v))
            out.append(buf.value)
    return b"\n".join(out) + b"\n"


def pad3(x):
    """a float array padded with zeros to a multiple of three: the vertices of a crafted mesh"""
    x = np.asarray(x, np.float32).reshape(-1)
    return np.concatenate([x, np.zeros((-x.size) % 3, np.float32)]).reshape(-1, 3)


def v_lines_to_floats(obj):
    """the values of the `v` lines of an .obj whose only sections are the header and `v`, one per line"""
    lines = obj.split(b"\n")
    assert lines[0].startswith(b"mtllib ") and lines[-1] == b""
    vals = []
    for ln in lines[1:-1]:
        parts = ln.split(b" ")
        assert parts[0] == b"v" and len(parts) == 4, ln
        vals.extend(parts[1:])
    return b"\n".join(vals) + b"\n"


# ---- crafted text-only atlas sets ----

def crafted_atlases(rng, n_mesh_faces, faces_per_atlas, coords_per_atlas):
    """an atlas set without images: atlas a lists faces_per_atlas[a] random mesh faces and owns coords_per_atlas[a] random coordinates, every
    corner a random id within the atlas (atlases with faces need at least one coordinate)"""
    nf = np.asarray(faces_per_atlas, np.int64); nc = np.asarray(coords_per_atlas, np.int64)
    assert np.all((nf == 0) | (nc > 0))
    face_ptr = np.concatenate([[0], np.cumsum(nf)]).astype(np.uint32); tc_ptr = np.concatenate([[0], np.cumsum(nc)]).astype(np.uint32)
    L, NM = int(face_ptr[-1]), int(tc_ptr[-1])
    faces = rng.integers(0, max(n_mesh_faces, 1), L).astype(np.uint32)
    ids = np.zeros((L, 3), np.uint32)
    for a in range(len(nf)):
        if nf[a]:
            ids[face_ptr[a]:face_ptr[a + 1]] = rng.integers(0, nc[a], (int(nf[a]), 3))
    merged = rng.uniform(0, 1, (NM, 2)).astype(np.float32)
    return dict(face_ptr=face_ptr, faces=faces, tc_ptr=tc_ptr, texcoords_merged=merged, texcoord_ids=ids)


# ---- the grammar of item 1, line by line ----

_FLOAT = rb"-?(?:\d+\.\d{6}|inf|nan)"
_RE = {k: re.compile(v) for k, v in dict(
    mtllib=rb"mtllib [^\n]*\.mtl", v=rb"v " + _FLOAT + b" " + _FLOAT + b" " + _FLOAT, vt=rb"vt " + _FLOAT + b" " + _FLOAT,
    vn=rb"vn " + _FLOAT + b" " + _FLOAT + b" " + _FLOAT, usemtl=rb"usemtl material(\d{4,})",
    f3=rb"f (\d+)/(\d+)/(\d+) (\d+)/(\d+)/(\d+) (\d+)/(\d+)/(\d+)", f2=rb"f (\d+)/(\d+) (\d+)/(\d+) (\d+)/(\d+)").items()}


def parse_obj(obj):
    """checks the text against the grammar and the order of the sections, every index against its section's count; returns the counts"""
    assert obj.endswith(b"\n")
    lines = obj[:-1].split(b"\n")
    assert _RE["mtllib"].fullmatch(lines[0])
    order = {"v": 0, "vt": 1, "vn": 2, "usemtl": 3, "f": 3}
    stage, n = 0, dict(v=0, vt=0, vn=0, usemtl=0, f=0)
    face_idx = []
    for ln in lines[1:]:
        kind = ln.split(b" ", 1)[0].decode()
        assert kind in order and order[kind] >= stage, ln
        stage = order[kind]
        if kind == "f":
            assert n["usemtl"] > 0
            m = _RE["f3"].fullmatch(ln) or _RE["f2"].fullmatch(ln)
            assert m, ln
            g = [int(x) for x in m.groups()]
            assert all(not s.startswith(b"0") for s in m.groups())
            face_idx.append((len(g) // 3, g))
        else:
            m = _RE[kind].fullmatch(ln)
            assert m, ln
            if kind == "usemtl":
                assert int(m.group(1)) == n["usemtl"] and (len(m.group(1)) == 4 or not m.group(1).startswith(b"0"))
        n[kind] += 1
    for per, g in face_idx:
        assert per == (3 if n["vn"] else 2)
        for k in range(3):
            c = g[per * k: per * k + per]
            assert 1 <= c[0] <= n["v"] and 1 <= c[1] <= n["vt"]
            if per == 3:
                assert c[2] == c[0] and c[2] <= n["vn"]
    return n


# ---- PNG decoding with the standard library ----

def decode_png(data):
    """(H, W, 3) uint8 of an 8-bit RGB, non-interlaced PNG whose rows all use filter 0; checks the signature, every chunk's CRC and (through
    zlib) the Adler-32 sum; returns (image, list of chunk types)"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks, idat, ihdr = 8, [], b"", None
    while at < len(data):
        n, typ = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert zlib.crc32(typ + body) & 0xFFFFFFFF == crc, typ
        chunks.append(typ)
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        at += 12 + n
    assert at == len(data) and chunks[0] == b"IHDR" and chunks[-1] == b"IEND"
    w, h, depth, colour, comp, filt, interlace = ihdr
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(idat)                     # raises on a wrong Adler-32
    assert len(raw) == h * (3 * w + 1)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3).copy(), chunks
