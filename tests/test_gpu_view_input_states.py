"""What a view input leaves behind (DESIGN.md section 4 "Shared plumbing of the view input"; csrc/view_input.h view_input_begin /
view_input_commit): ONE rule for the four ways in.  After a refused call the context has no views -- a data-cost pass, the read-back of a
view's image and set_view_masks are MVS_ERR_STATE, n_views is 0 -- until a view input succeeds, which then gives the same table bit for
bit; a successful call with zero views still gives the empty table.

The refused call brings FEWER views than the good one before it, and its last view is the bad one: a width of 1 where the views bring
pixels, a frame that has not the view's size where they bring files.  (A context that kept the old count next to the new, shorter view
table would walk off that table in the next pass; the refused call itself fails on the host, before anything is launched.)"""
import numpy as np
import pytest

import mvs_texturing_amd as M
import jpeg_full_decode as FD
from conftest import get_scene

pytestmark = pytest.mark.gpu

MVS_ERR_STATE = 6
LENS = {0: (0.9, -0.2, 0.05), 3: (1.1, -0.12, 0.0)}
FEWER = 4                                                  # views of the refused call; its last one is bad


@pytest.fixture(scope="module")
def files():
    return [FD.pillow_file(img, quality=90, subsampling=2) for img in get_scene("tiny").images]


def _cams(s, n, **last):
    """the first n cameras, with fields of the last one replaced"""
    cams = {k: np.array(v[:n]) for k, v in s.cams.items()}
    for k, v in last.items():
        cams[k][n - 1] = v
    return cams


def _lens(n):
    rows = np.zeros((n, 3), np.float32)
    rows[:, 0] = 1.0
    for j, l in LENS.items():
        if j < n:
            rows[j] = l
    return rows


def _pixels(s, n, narrow_last=False):
    """the first n images; narrow_last: the last one 1 pixel wide, as its camera then says"""
    images = list(s.images[:n])
    if narrow_last:
        images[-1] = np.ascontiguousarray(images[-1][:, :1])
    return images


# way -> (good or empty call with n views, refused call)
WAYS = {
    "set_views": (lambda c, s, f, n: c.set_views(_cams(s, n), _pixels(s, n)),
                  lambda c, s, f: c.set_views(_cams(s, FEWER, width=1), _pixels(s, FEWER, True))),
    "set_views_jpeg": (lambda c, s, f, n: c.set_views_jpeg(_cams(s, n), f[:n]),
                       lambda c, s, f: c.set_views_jpeg(_cams(s, FEWER, width=160), f[:FEWER])),
    "set_views_lens": (lambda c, s, f, n: c.set_views(_cams(s, n), _pixels(s, n), lens=_lens(n)),
                       lambda c, s, f: c.set_views(_cams(s, FEWER, width=1), _pixels(s, FEWER, True), lens=_lens(FEWER))),
    "set_views_jpeg_lens": (lambda c, s, f, n: c.set_views_jpeg(_cams(s, n), f[:n], lens=_lens(n)),
                            lambda c, s, f: c.set_views_jpeg(_cams(s, FEWER, width=160), f[:FEWER], lens=_lens(FEWER))),
}


def _table(c):
    c.data_costs(M.Settings())
    return c.costs_download()


def _same_table(a, b):
    assert a.n_faces == b.n_faces and a.n_views == b.n_views and a.nnz == b.nnz
    assert np.array_equal(a.col_ptr, b.col_ptr) and np.array_equal(a.view_id, b.view_id)
    assert np.array_equal(np.asarray(a.cost).view(np.uint32), np.asarray(b.cost).view(np.uint32))


@pytest.mark.parametrize("way", sorted(WAYS))
def test_refusal_leaves_no_views(way, files):
    s = get_scene("tiny")
    good, refused = WAYS[way]
    assert FEWER < s.n_views
    c = M.Context(0)
    try:
        c.set_mesh(s.verts, s.faces, s.normals)
        good(c, s, files, s.n_views)                                              # 1. a good call, then the table
        first = _table(c)
        assert c.n_views == s.n_views and first.nnz > 0
        with pytest.raises(M.MvsError) as e:                                      # 2. fewer views, the last one bad
            refused(c, s, files)
        assert e.value.status == 1 and "view %d" % (FEWER - 1) in str(e.value), str(e.value)
        assert ("bad image" if "jpeg" not in way else "the frame is 320 x 240, the view 160 x 240") in str(e.value), str(e.value)
        with pytest.raises(M.MvsError) as e:                                      # 3. the context has no views
            c.data_costs(M.Settings())
        assert e.value.status == MVS_ERR_STATE and "the last view input was refused" in str(e.value), str(e.value)
        with pytest.raises(M.MvsError) as e:
            c.view_image(0)
        assert e.value.status == MVS_ERR_STATE, str(e.value)
        with pytest.raises(M.MvsError) as e:
            c.set_view_masks([np.ones((240, 320), np.uint8)] * FEWER)
        assert e.value.status == MVS_ERR_STATE and "no views" in str(e.value), str(e.value)
        assert c.n_views == 0
        good(c, s, files, s.n_views)                                              # 4. the good call again: the first table, bit for bit
        assert c.n_views == s.n_views
        _same_table(_table(c), first)
        good(c, s, files, 0)                                                      # 5. zero views is no refusal: the empty table
        empty = _table(c)
        assert c.n_views == 0 and empty.nnz == 0 and empty.n_faces == s.n_faces and (np.asarray(empty.col_ptr) == 0).all()
    finally:
        c.close()
