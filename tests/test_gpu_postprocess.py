"""mvs_postprocess_face_infos on the device -- outlier_kernel (LDS-staged and from global memory), nonzero_count / nonzero_copy,
sort_columns, max, hist, percentile and cost kernels of csrc/k_dc.hip -- against the plain reference of the whole stage
(tests/tools/postprocess_model.py, itself equal to upstream's compiled function on every case: tests/test_postprocess_model.py), on
crafted inputs that take every exit of the outlier loop in neighbouring lanes and every seam of the launch shapes."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import postprocess_model as PM

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.float32(x).view(np.uint32)


def _device(c, mode_name):
    return M.viewsel.postprocess_face_infos(*c.args(), M.Settings(outlier_removal=mode_name))


def _compare(c, mode, got, st):
    """pattern, view ids, nnz, maximum and percentile exact; costs bit for bit"""
    name = "%s/%s" % (c.name, PM.MODES[mode][1])
    col_ptr, view, cost, q, rc, mx, pct, _ = PM.reference_of(c.name, mode)
    assert got.nnz == len(view) == st["nnz"], name
    assert np.array_equal(got.col_ptr, col_ptr), name
    assert np.array_equal(got.view_id, view), name
    assert _bits(st["max_quality"]) == _bits(mx), (name, st["max_quality"], mx)
    assert _bits(st["percentile"]) == _bits(pct), (name, st["percentile"], pct)
    differ = np.nonzero(got.cost.view(np.uint32) != cost.view(np.uint32))[0]
    print("%s: nnz %d, costs that differ from the reference in bits: %d" % (name, got.nnz, len(differ)))
    assert len(differ) == 0, (name, differ[:8], got.cost[differ[:8]], cost[differ[:8]])


@pytest.mark.parametrize("name", PM.CASE_NAMES)
def test_crafted_case_equals_the_reference(name):
    """every case of postprocess_cases() in all three outlier modes: col_ptr, view ids, nnz, the maximum and the percentile (as float
    bits) and every cost, bit for bit -- under gauss_damping too, where an fp64 exp (OCML's on the device, glibc's in the reference)
    reaches the output: costs that differ there, measured on an MI355X over all cases: 0."""
    c = PM.get_case(name)
    for mode, mode_name in PM.MODES:
        got, st = _device(c, mode_name)
        _compare(c, mode, got, st)


def test_handover_between_the_lds_and_the_global_memory_kernel():
    """the same 500 faces and one more: with 78 infos the longest column still fits the LDS staging of outlier_kernel<true>, with 79
    and with 300 it does not and outlier_kernel<false> runs every face (launch_outlier: LDS_PER_ENTRY = 64 * (3 * 4 + 1) = 832 bytes
    per entry, 64 KB / 832 = 78).  The shared faces give the same columns and costs in the three calls, each equal to the reference."""
    limit = (64 * 1024) // (64 * (3 * 4 + 1))                 # launch_outlier: the longest column the LDS-staged kernel takes
    assert limit == PM.LDS_MAX_COLUMN == 78
    cases = [PM.get_case("handover_%d" % n) for n in (limit, limit + 1, 300)]
    for mode, mode_name in PM.MODES:
        res = []
        for c in cases:
            assert int(np.diff(c.info_ptr.astype(np.int64)).max()) == int(c.name.split("_")[1])
            got, st = _device(c, mode_name)
            _compare(c, mode, got, st)
            res.append(got)
        s = cases[0].info["shared"]
        e = int(res[0].col_ptr[s])
        for got in res[1:]:
            assert np.array_equal(got.col_ptr[:s + 1], res[0].col_ptr[:s + 1]) and np.array_equal(got.view_id[:e], res[0].view_id[:e]), mode_name
            assert np.array_equal(got.cost[:e].view(np.uint32), res[0].cost[:e].view(np.uint32)), mode_name


def test_refused_inputs_return_their_status_and_leave_the_next_call_intact():
    """a descending info_ptr, a view id >= n_views, an outlier mode without colours, 65536 views: each returns its status, and a
    correct call right after it gives the reference's result"""
    c = PM.get_case("faces_65")
    V, ptr, view, q, col = c.args()
    bad_ptr = ptr.copy(); bad_ptr[2] = ptr[-1]                # descends at face 2, every entry still inside the arrays
    assert bad_ptr[3] < bad_ptr[2]
    clamp = M.Settings(outlier_removal="gauss_clamping")
    refused = [("descending info_ptr", (V, bad_ptr, view, q, col, clamp), 1),
               ("view id >= n_views", (int(view.max()), ptr, view, q, col, clamp), 1),
               ("outlier mode without colours", (V, ptr, view, q, None, clamp), 1),
               ("65536 views", (65536, ptr, view, q, col, clamp), 3)]
    for what, args, status in refused:
        with pytest.raises(M.viewsel.MvsError) as e:
            M.viewsel.postprocess_face_infos(*args)
        assert e.value.status == status, (what, str(e.value))
        got, st = _device(c, "gauss_clamping")
        _compare(c, 2, got, st)
