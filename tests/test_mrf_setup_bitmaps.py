"""The solver's set-up from per-face view bitmaps (k_mrf_setup.hip mrf_bitmap_kernel, mrf_record_bits_kernel, mrf_map_bits_kernel; the
arithmetic in dmath.h "view-set bitmaps").

A column's view ids are strictly ascending (calculate_data_costs.cpp:272), so a column is a bitmap: two columns are identical iff
their bitmaps are equal, and the position of a view in a column is the number of set bits below it.  Host tests: those identities
against plain list search.  GPU tests: the records, descriptors and identity flags of the bitmap route against those of the list
route byte for byte, the solver's results against the oracle, and tables that break the rule (they must take the list route)."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
from conftest import get_scene
from util_cases import random_mrf, random_mrf_mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _dmath():
    D = C.CDLL(os.path.join(ROOT, "mvs-texturing_amd", "csrc", "libmvs_dmath_host.so"))
    D.dmh_bitmap_words.restype = C.c_uint32; D.dmh_bitmap_words.argtypes = [C.c_uint32]
    D.dmh_bitmap_of_list.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    D.dmh_bitmap_rank.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    D.dmh_bitmap_equal.restype = C.c_int; D.dmh_bitmap_equal.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    D.dmh_bitmap_select.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    return D


def _bitmap(D, lst, V):
    lst = np.ascontiguousarray(lst, dtype=np.uint16)
    bits = np.zeros(max(int(D.dmh_bitmap_words(V)), 1), dtype=np.uint64)
    D.dmh_bitmap_of_list(lst.ctypes.data, len(lst), V, bits.ctypes.data)
    return bits


def _check_pair(D, a, b, V):
    """every question the set-up asks about the lists a (own) and b (neighbour), from their bitmaps, against the lists themselves"""
    W = int(D.dmh_bitmap_words(V))
    assert W == (V + 63) // 64
    ba, bb = _bitmap(D, a, V), _bitmap(D, b, V)
    assert bool(D.dmh_bitmap_equal(ba.ctypes.data, bb.ctypes.data, W)) == (list(a) == list(b))
    q = np.arange(V, dtype=np.uint32)                      # position of every view in a: lower-bound search on the list
    got = np.zeros(V, dtype=np.uint32)
    D.dmh_bitmap_rank(ba.ctypes.data, W, q.ctypes.data, V, got.ctypes.data)
    a64 = np.asarray(a, dtype=np.int64)
    lo = np.searchsorted(a64, q.astype(np.int64))
    found = (lo < len(a64)) & (a64[np.minimum(lo, max(len(a64) - 1, 0))] == q) if len(a64) else np.zeros(V, bool)
    want = np.where(found, lo, NONE).astype(np.uint32)
    assert np.array_equal(got, want)
    sel = np.zeros(len(b), dtype=np.uint32)                # the neighbour's labels enumerated from its bitmap = its list
    D.dmh_bitmap_select(bb.ctypes.data, W, len(b), sel.ctypes.data)
    assert np.array_equal(sel, np.asarray(b, dtype=np.uint32))


def test_bitmap_rank_identity_select_against_list_search():
    D = _dmath()
    for V in (1, 63, 64, 65, 128, 130, 200, 700, 1000, 1024):
        full = list(range(V))
        edge_ids = sorted({v for v in (0, 62, 63, 64, 65, 127, 128, V - 2, V - 1) if 0 <= v < V})
        cases = [([], []), ([], full), (full, []), (full, full), ([V - 1], [V - 1]), ([0], [V - 1]), (edge_ids, edge_ids), (edge_ids, full),
                 (full[::2], full[1::2]),                  # disjoint
                 (full[::3], full),                        # subset
                 (full, full[::3]),
                 ([v for v in full if v // 64 == (V - 1) // 64], [v for v in full if v // 64 == 0])]   # only the last word / only the first
        for a, b in cases:
            _check_pair(D, a, b, V)
    rng = np.random.default_rng(5)
    for _ in range(300):
        V = int(rng.integers(1, 1025))
        ka, kb = int(rng.integers(0, min(V, 255) + 1)), int(rng.integers(0, min(V, 255) + 1))
        a = np.sort(rng.choice(V, ka, replace=False)); b = np.sort(rng.choice(V, kb, replace=False))
        if rng.random() < 0.3:
            b = a.copy()
        _check_pair(D, a.tolist(), b.tolist(), V)


def test_bitmap_of_list_drops_ids_beyond_the_views():
    """an id >= n_views must not set a bit outside the face's words (mrf_bitmap_kernel checks the bound the same way)"""
    D = _dmath()
    lst = np.array([3, 64, 130, 200, 65535], dtype=np.uint16)
    for V, word2 in ((130, 0), (131, 1 << 2)):             # three words each; the fourth is not the face's
        bits = np.full(4, 0xDEADBEEF, dtype=np.uint64)
        D.dmh_bitmap_of_list(lst.ctypes.data, len(lst), V, bits.ctypes.data)
        assert bits.tolist() == [1 << 3, 1, word2, 0xDEADBEEF]


# ---- GPU ----
def _solve(table, adj_ptr, adj, params, force_lists, prune=0, tables=True):
    n, V, col_ptr, view_id, cost = table
    c = M.Context(0)
    try:
        if force_lists is not None:                         # (None: no option set, the set-up decides)
            c.set_option("mrf_force_lists", force_lists)
        c.costs_upload(M.viewsel.DataCosts(n, V, col_ptr, view_id, cost))
        if prune:
            c.prune_labels(prune)
        labels, st = c.view_selection(adj_ptr, adj, M.viewsel.default_mrf_params(**params))
        return labels, st, (c.mrf_setup_tables() if tables else None)
    finally:
        c.close()


_case_cache = {}


def _case(name):
    """name -> ((n, V, col_ptr, view_id, cost), adj_ptr, adj, prune, the table the oracle solves)"""
    if name in _case_cache:
        return _case_cache[name]
    prune = 0
    if name in ("bumpy", "pruned", "manyviews"):
        s = get_scene("manyviews" if name == "manyviews" else "bumpy")
        ref, _ = O.data_costs(s)
        t = (ref.n_faces, ref.n_views, ref.col_ptr, ref.view_id, ref.cost); adj_ptr, adj = s.adj_ptr, s.adj
        if name == "pruned":
            prune = 3; ref = O.prune_labels(ref, prune)
    elif name == "config2":                                # BASELINE config 2; its table from the device (the data costs have their own tests)
        s = M.synth.make_scene(**M.synth.CONFIGS[2])
        c = M.Context(0)
        try:
            c.set_mesh(s.verts, s.faces, s.normals); c.set_views(s.cams, s.images); c.data_costs(M.Settings()); dc = c.costs_download()
        finally:
            c.close()
        t = (dc.n_faces, dc.n_views, dc.col_ptr, dc.view_id, dc.cost); adj_ptr, adj = s.adj_ptr, s.adj
        ref = O.CsrNp(*t)
    else:
        if name == "mixed":                                # hubs of degree up to 6, empty columns, columns beyond 255 labels (generic nodes beside fast ones)
            n, V = 6000, 400; tab = random_mrf_mixed(n, V, 11)
        elif name == "v130":                               # V no multiple of 64, dense columns: many views in the last, partial word
            n, V = 4000, 130; tab = random_mrf(n, V, 60, 3, 21, 0.1)
        else:                                              # "v65": one view in the second word
            n, V = 3000, 65; tab = random_mrf(n, V, 30, 3, 22, 0.05)
        col_ptr, view_id, cost, adj_ptr, adj = tab
        t = (n, V, col_ptr, view_id, cost); ref = O.CsrNp(*t)
    _case_cache[name] = (t, adj_ptr, adj, prune, ref)
    return _case_cache[name]


CASES = ["bumpy", "config2", "mixed", "pruned", "manyviews", "v130", "v65"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_bitmap_route_builds_the_list_routes_bytes(name):
    """records, descriptors and identity flags of the bitmap route == those of the list route (the kernels the bitmap route replaces,
    forced by the "mrf_force_lists" hook), byte for byte; so are labels and statistics"""
    t, adj_ptr, adj, prune, _ = _case(name)
    l0, s0, t0 = _solve(t, adj_ptr, adj, {}, 1, prune)
    l1, s1, t1 = _solve(t, adj_ptr, adj, {}, 0, prune)
    assert not t0["bitmaps"] and t1["bitmaps"]
    print(name, "faces", t[0], "views", t[1], "edges", len(adj), "identical", int(t0["ident"].sum()), "fast nodes", t0["desc"].shape[0], "record words", t0["rec"].size)
    assert t0["ident"].size == len(adj) and t0["desc"].shape[0] > 0 and t0["rec"].size > 256
    if name in ("bumpy", "config2"):
        assert 0 < int(t0["ident"].sum()) < (t0["ident"].size)          # both kinds of edge occur
    for k in ("ident", "desc", "rec"):
        assert t0[k].shape == t1[k].shape, k
        bad = np.nonzero(t0[k].ravel() != t1[k].ravel())[0]
        assert bad.size == 0, "%s differs at %d places, first at %d" % (k, bad.size, bad[0])
    assert np.array_equal(l0, l1)
    for k in ("energy_fixed", "sweeps", "icm_iters"):
        assert s0[k] == s1[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_bitmap_route_results_equal_the_oracle(name):
    """labels, energy, sweeps and ICM rounds against the oracle: ICM only, sweep 1 alone, the hand-over to the replayed graph after
    sweep 4, one sweep beyond it, and the default stop rule"""
    t, adj_ptr, adj, prune, ref = _case(name)
    for p in (dict(max_sweeps=0, min_sweeps=0), dict(max_sweeps=1, min_sweeps=1), dict(max_sweeps=4, min_sweeps=4), dict(max_sweeps=5, min_sweeps=5), dict()):
        lo, so = O.view_selection(ref, adj_ptr, adj, O.default_mrf_params(**p))
        lg, sg, tb = _solve(t, adj_ptr, adj, p, 0, prune, tables=True)
        assert tb["bitmaps"]
        assert np.array_equal(lo, lg), p
        assert (so["energy_fixed"], so["sweeps"], so["icm_iters"]) == (sg["energy_fixed"], sg["sweeps"], sg["icm_iters"]), p


@pytest.mark.gpu
def test_generic_senders_maps_from_bitmaps():
    """every node on the generic kernel (16-bit maps of mrf_map_bits_kernel instead of mrf_map_kernel): same results on both routes and the oracle's"""
    t, adj_ptr, adj, prune, ref = _case("mixed")
    lo, so = O.view_selection(ref, adj_ptr, adj)
    n, V, col_ptr, view_id, cost = t
    for force_lists in (1, 0):
        c = M.Context(0)
        try:
            c.set_option("mrf_force_lists", force_lists); c.set_option("mrf_force_generic", 1)
            c.costs_upload(M.viewsel.DataCosts(n, V, col_ptr, view_id, cost))
            lg, sg = c.view_selection(adj_ptr, adj)
            assert c.mrf_setup_tables()["bitmaps"] == (not force_lists)
        finally:
            c.close()
        assert np.array_equal(lo, lg)
        assert (so["energy_fixed"], so["sweeps"], so["icm_iters"]) == (sg["energy_fixed"], sg["sweeps"], sg["icm_iters"])


@pytest.mark.gpu
def test_route_decision_at_1024_views():
    """the set-up's own choice of route on both sides of its boundary, W = ceil(V / 64) <= 16 words: bitmaps at V = 1024, lists at
    V = 1025 with no option set (the 1025 instance has entries with id 1024, the seventeenth word); at both, the oracle's results, and
    the same records, descriptors and identity flags whichever route is forced"""
    n = 600
    for V in (1024, 1025):
        col_ptr, view_id, cost, adj_ptr, adj = random_mrf(n, V, 40, 3, 31, 0.05)
        t = (n, V, col_ptr, view_id, cost)
        if V == 1025:
            assert int((np.asarray(view_id) == 1024).sum()) == 10
        lo, so = O.view_selection(O.CsrNp(*t), adj_ptr, adj)
        ld, sd, td = _solve(t, adj_ptr, adj, {}, None)
        assert bool(td["bitmaps"]) == (V == 1024), V
        l0, s0, t0 = _solve(t, adj_ptr, adj, {}, 0)
        l1, s1, t1 = _solve(t, adj_ptr, adj, {}, 1)
        assert bool(t0["bitmaps"]) == (V == 1024) and not t1["bitmaps"], V
        print(V, "bitmaps", bool(td["bitmaps"]), "sweeps", sd["sweeps"], "fast nodes", td["desc"].shape[0], "record words", td["rec"].size)
        for lg, sg in ((ld, sd), (l0, s0), (l1, s1)):
            assert np.array_equal(lo, lg), V
            assert (so["energy_fixed"], so["sweeps"], so["icm_iters"]) == (sg["energy_fixed"], sg["sweeps"], sg["icm_iters"]), V
        for k in ("rec", "desc", "ident"):
            assert t0[k].shape == t1[k].shape and t0[k].tobytes() == t1[k].tobytes(), (V, k)
            assert td[k].tobytes() == t0[k].tobytes(), (V, k)


def broken_tables():
    """name -> (table, adj_ptr, adj): the "v130" table with ONE column that breaks the rule the bitmaps rest on"""
    (n, V, col_ptr, view_id, cost), adj_ptr, adj, _, _ = _case("v130")
    K = np.diff(col_ptr.astype(np.int64))
    i = int(np.nonzero(K >= 5)[0][7]); a = int(col_ptr[i])
    out = {}
    v = view_id.copy(); v[a + 1], v[a + 2] = v[a + 2], v[a + 1]; out["swapped_pair"] = v
    v = view_id.copy(); v[a + 3], v[a + 4] = v[a + 4], v[a + 3]; out["swapped_pair_across_lanes"] = v   # entries 3 | 4: two lanes of the bitmap kernel
    v = view_id.copy(); v[a + 2] = v[a + 1]; out["duplicate"] = v
    v = view_id.copy(); v[a + K[i] - 1] = V; out["id_equals_n_views"] = v
    return {k: ((n, V, col_ptr, v, cost), adj_ptr, adj) for k, v in out.items()}


# crc32 of the labels, energy_fixed, sweeps, icm_iters of the commit before the bitmap route existed (one route, the list kernels)
BROKEN_PINS = {
    "swapped_pair": (1985554679, 14830178850928, 20, 1),
    "duplicate": (1985554679, 14830178850928, 20, 1),
    "swapped_pair_across_lanes": (1985554679, 14830178850928, 20, 1),
    "id_equals_n_views": (1985554679, 14830178850928, 20, 1),
}


def outcome(labels, st):
    return (zlib.crc32(np.ascontiguousarray(labels, dtype=np.uint32).tobytes()), int(st["energy_fixed"]), int(st["sweeps"]), int(st["icm_iters"]))


def solve_outcome(table, adj_ptr, adj, force_lists=None):
    """(outcome or ("error", status), set-up tables or None) of one solve in a context of its own"""
    n, V, col_ptr, view_id, cost = table
    c = M.Context(0)
    try:
        if force_lists is not None:
            c.set_option("mrf_force_lists", force_lists)
        c.costs_upload(M.viewsel.DataCosts(n, V, col_ptr, view_id, cost))
        labels, st = c.view_selection(adj_ptr, adj)
        return outcome(labels, st), (c.mrf_setup_tables() if force_lists is not None else None)
    except M.viewsel.MvsError as e:
        return ("error", int(getattr(e, "status", -1))), None
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BROKEN_PINS))
def test_table_that_is_not_strictly_ascending_takes_the_list_route(name):
    """a caller's table (mvs_ctx_costs_upload takes it as it is) with a swapped pair, a duplicate or an id = n_views in one column: the
    bitmap kernel flags it, the set-up keeps to the list kernels, and the outcome is what it was before the bitmap route existed"""
    t, adj_ptr, adj = broken_tables()[name]
    o1, t1 = solve_outcome(t, adj_ptr, adj, 0)
    o0, t0 = solve_outcome(t, adj_ptr, adj, 1)
    print(name, o1)
    assert o1 == o0
    if t1 is not None:
        assert not t1["bitmaps"] and not t0["bitmaps"]
        for k in ("ident", "desc", "rec"):
            assert np.array_equal(t0[k], t1[k]), k
    assert o1 == BROKEN_PINS[name]
