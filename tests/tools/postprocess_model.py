"""A plain reference of tex::postprocess_face_infos (calculate_data_costs.cpp:253-306) composed from the oracle's single-face
outlier detection and its histogram percentile, and crafted inputs for mvs_postprocess_face_infos (tests/test_postprocess_model.py
checks the composition against upstream's own compiled function on every case; tests/test_gpu_postprocess.py compares the device
with it).  Nothing here calls the library under test.

The composition, in upstream's order: orc_outlier_detection per face on the infos in the order given; erase quality == 0 (outlier
modes only); sort each face by view id; max; orc_percentile(., 0.995); cost = 1 - min(1, q / p) in fp32.

Inputs left out on purpose: any input whose surviving qualities are all zero while nnz > 0 (mode `none` with only zero qualities:
upstream indexes its histogram with NaN there, the behaviour is undefined), and negative qualities.  View ids are distinct within
a face (std::sort leaves the order of equal ids open)."""
import ctypes as C
import functools

import numpy as np

import oracle_py as O

MODES = ((0, "none"), (1, "gauss_damping"), (2, "gauss_clamping"))
# the exit photometric_outlier_detection took (orc_outlier_detection_trace, trace[0])
EXIT_NOTHING, EXIT_FEW_INLIERS, EXIT_SMALL_COVARIANCE, EXIT_NOT_INVERTIBLE, EXIT_TEN_ROUNDS = 0, 1, 2, 3, 4
EXIT_NAMES = ("nothing to do", "fewer than 4 inliers", "covariance below 5e-4", "not invertible", "ten rounds")

# launch_outlier (csrc/k_dc.hip): the colours and inlier flags of a block's 64 faces are staged into LDS when the longest column
# fits into 64 KB -- LDS_PER_ENTRY = 64 faces x (three floats + the inlier flag); longer columns take the global-memory kernel
LDS_PER_ENTRY = 64 * (3 * 4 + 1)
LDS_MAX_COLUMN = (64 * 1024) // LDS_PER_ENTRY


def _lib():
    L = O.load()
    L.orc_outlier_detection_trace.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.orc_outlier_detection_trace.restype = C.c_int
    return L


def outlier_face(color, quality, mode):
    """the oracle's photometric_outlier_detection on one face: (return code, qualities after it, trace[4])"""
    L = _lib()
    color = np.ascontiguousarray(color, np.float32); q = np.array(quality, np.float32)
    trace = np.zeros(4, np.int32)
    rc = L.orc_outlier_detection_trace(len(q), color.ctypes.data, q.ctypes.data, int(mode), trace.ctypes.data)
    return rc, q, trace


def postprocess_reference_traced(n_views, info_ptr, view_id, quality, mean_color, mode):
    """postprocess_reference and, per face, the exit the outlier detection took: an (F, 4) array of traces"""
    L = _lib()
    ptr = np.ascontiguousarray(info_ptr, np.uint32).astype(np.int64)
    F, n = len(ptr) - 1, int(ptr[-1])
    view = np.ascontiguousarray(view_id, np.uint16)
    q = np.array(quality, np.float32)                       # a copy: the detection writes into it
    rc = np.ones(F, np.int32); trace = np.zeros((F, 4), np.int32)
    assert n == 0 or int(view.max()) < n_views
    if mode:
        col = np.ascontiguousarray(mean_color, np.float32).reshape(-1, 3)
        cp, qp, tp = col.ctypes.data, q.ctypes.data, trace.ctypes.data
        for i in range(F):
            a, b = int(ptr[i]), int(ptr[i + 1])
            rc[i] = L.orc_outlier_detection_trace(b - a, cp + 12 * a, qp + 4 * a, int(mode), tp + 16 * i)
    keep = (q != 0) if mode else np.ones(n, bool)           # (:268-270; a NaN quality stays, as NaN == 0 is false)
    face = np.repeat(np.arange(F), np.diff(ptr))
    idx = np.nonzero(keep)[0]
    idx = idx[np.lexsort((view[idx], face[idx]))]           # by face, inside a face by view id (:272)
    col_ptr = np.zeros(F + 1, np.uint32); col_ptr[1:] = np.cumsum(np.bincount(face[idx], minlength=F))
    qs = q[idx]
    mx = np.float32(0.0)
    if len(qs):                                             # std::max(max, q) over the infos (:278-281): a NaN never replaces the maximum
        mx = np.float32(np.fmax.reduce(qs, initial=np.float32(0.0)))
    pct = np.float32(L.orc_percentile(qs.ctypes.data, len(qs), C.c_float(float(mx)), C.c_float(0.995)))
    with np.errstate(all="ignore"):
        nq = (qs / pct).astype(np.float32)
        nq = np.where(nq < np.float32(1.0), nq, np.float32(1.0)).astype(np.float32)     # std::min(1.0f, x): x only if x < 1
        cost = (np.float32(1.0) - nq).astype(np.float32)
    return col_ptr, view[idx].copy(), cost, qs, rc, mx, pct, trace


def postprocess_reference(n_views, info_ptr, view_id, quality, mean_color, mode):
    """(col_ptr, view_id, cost, quality, per-face return codes, max_quality, percentile) of tex::postprocess_face_infos on infos in
    CSR by face, mode 0 none / 1 gauss_damping / 2 gauss_clamping"""
    return postprocess_reference_traced(n_views, info_ptr, view_id, quality, mean_color, mode)[:7]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """one complete input of mvs_postprocess_face_infos.  `family[i]` names the family face i belongs to; `outlier` says whether the
    case is one of the outlier-loop cases (input qualities in [0.8, 1]); `info` holds what a family wants checked."""
    def __init__(self, name, n_views, info_ptr, view_id, quality, mean_color, family, outlier=False, info=None):
        self.name, self.n_views, self.outlier, self.info = name, int(n_views), outlier, info or {}
        self.info_ptr = np.ascontiguousarray(info_ptr, np.uint32); self.view_id = np.ascontiguousarray(view_id, np.uint16)
        self.quality = np.ascontiguousarray(quality, np.float32); self.mean_color = np.ascontiguousarray(mean_color, np.float32).reshape(-1, 3)
        self.family = np.array(family, dtype="U16")
        assert len(self.family) == self.n_faces and len(self.view_id) == len(self.quality) == len(self.mean_color) == self.n_infos
        assert self.n_infos <= 100000 and not (self.quality < 0).any()

    @property
    def n_faces(self):
        return len(self.info_ptr) - 1

    @property
    def n_infos(self):
        return int(self.info_ptr[-1])

    def args(self):
        return self.n_views, self.info_ptr, self.view_id, self.quality, self.mean_color

    def faces_of(self, family):
        return np.nonzero(self.family == family)[0]


def _pack(name, faces, rng, n_views=None, interleave=True, order=None, **kw):
    """faces = [(colours (n, 3), qualities (n), family)] -> Case; the faces in a seeded random order (families interleaved face by
    face), view ids distinct per face and shuffled, or order[i] in {"asc", "desc", "shuffled"}"""
    perm = rng.permutation(len(faces)) if interleave else np.arange(len(faces))
    faces = [faces[i] for i in perm]
    cnt = np.array([len(f[1]) for f in faces], np.int64)
    n_views = int(n_views or max(int(cnt.max()) if len(cnt) else 1, 100))
    ptr = np.zeros(len(faces) + 1, np.uint32); ptr[1:] = np.cumsum(cnt)
    views = []
    for k, c in enumerate(cnt):
        v = rng.permutation(n_views)[:c]
        o = order[perm[k]] if order is not None else "shuffled"
        views.append(np.sort(v) if o == "asc" else np.sort(v)[::-1] if o == "desc" else v)
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
    c = Case(name, n_views, ptr, cat(views, (0,), np.uint16), cat([np.asarray(f[1], np.float32) for f in faces], (0,), np.float32),
             cat([np.asarray(f[0], np.float32).reshape(-1, 3) for f in faces], (0, 3), np.float32), [f[2] for f in faces], **kw)
    c.perm = perm
    return c


def _q(rng, n):
    """input qualities of the outlier families: [0.8, 1.0], so that most costs fall into (0, 0.5] where 1 - q / p is exact"""
    return (np.float32(0.8) + rng.random(n).astype(np.float32) * np.float32(0.2)).astype(np.float32)


def _cluster(rng, n, sigma, n_out=0):
    col = (rng.random(3) * 0.6 + 0.2 + rng.standard_normal((n, 3)) * sigma).astype(np.float32)
    if n_out:
        col[rng.choice(n, n_out, replace=False)] = rng.random((n_out, 3)).astype(np.float32)
    return col


def _fam_lengths(rng):
    """every n mod 4 tail of the unrolled walks, the n < 4 return, columns at and next to 64 entries and at the LDS limit"""
    out = []
    for n in list(range(10)) + [63, 64, 65, LDS_MAX_COLUMN - 1, LDS_MAX_COLUMN]:
        for _ in range(6):
            out.append((_cluster(rng, n, 0.05, n // 6 if n >= 5 else 0), _q(rng, n), "lengths"))
    return out


def _fam_zero_covariance(rng):
    out = []
    for n in (4, 5, 6, 7, 9, 16, 33):                       # identical colours: zero covariance in the first round, nothing to zero
        for _ in range(3):
            out.append((np.tile(rng.random(3).astype(np.float32), (n, 1)), _q(rng, n), "zc_identical"))
    for k in range(80):                                     # a tight cluster and far outliers: rejected first, zeroed by a later round
        n = int(rng.integers(16, 41)); n_out = int(rng.integers(1, 4))
        sigma = 10.0 ** rng.uniform(np.log10(1e-4), np.log10(3e-3))
        col = _cluster(rng, n, sigma)
        far = rng.standard_normal((n_out, 3)); far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(0.3, 0.6, (n_out, 1))
        sel = rng.choice(n, n_out, replace=False)
        col[sel] = (col[sel] + far).astype(np.float32)
        out.append((col, _q(rng, n), "zc_tight"))
    return out


def rank_deficient_faces(rng, count=1040):
    """colours exactly collinear (c = o + a x) or coplanar (c = o + a x + b y) in float32: o, a, b multiples of 1/32 and x, y multiples
    of 1/64, so every product and sum is exact; general directions, not axis-aligned.  A third of the faces are left exact, the rest
    get 1..4 float ulps on a few coordinates.  The covariance is singular up to the rounding of the fp64 mean: the rank rule of the
    full-pivot LU decides by differences of 1e-16."""
    out = []
    for k in range(count):
        n = int(rng.choice([6, 7, 8, 9, 11, 12, 16, 20]))
        o = rng.integers(4, 12, 3) / 32.0
        a = rng.integers(-15, 16, 3) / 32.0; b = rng.integers(-15, 16, 3) / 32.0
        if not a.any():
            a[0] = 0.25
        x = rng.integers(0, 64, n) / 64.0; y = rng.integers(0, 64, n) / 64.0
        col = o + np.outer(x, a) + (np.outer(y, b) if k % 2 else 0.0)
        col32 = col.astype(np.float32)
        assert np.array_equal(col32.astype(np.float64), col)
        if k % 3:
            m = int(rng.integers(1, 4))
            for _ in range(m):
                i, ch = int(rng.integers(n)), int(rng.integers(3))
                col32.view(np.int32)[i, ch] += int(rng.integers(1, 5)) * (1 if rng.random() < 0.5 else -1)
        out.append((col32, _q(rng, n), "rank"))
    return out


def _fam_few_inliers(rng):
    """sets of 4..8 infos of which 2..5 are outliers.  (With the sample covariance of n points no point is further than
    (n - 1)^2 / n from the mean in squared Mahalanobis distance, below the threshold's 10.23 for n <= 12: such a set loses inliers
    only through rounding.  What the reference makes of these faces is counted by the tests, not assumed.)"""
    out = []
    for k in range(120):
        n = int(rng.integers(4, 9)); n_out = int(min(n, rng.integers(2, 6)))
        out.append((_cluster(rng, n, 10.0 ** rng.uniform(-3.5, -1.3), n_out), _q(rng, n), "few"))
    return out


def _fam_no_convergence(rng, want=12, tries=6000):
    """two-cluster mixtures of comparable weight on which the reference's tenth round still changes the inlier set, found by a seeded
    search with the reference itself (its trace says whether the last round changed a flag)"""
    out = []
    for _ in range(tries):
        n = int(rng.integers(20, 60)); n1 = int(n * rng.uniform(0.4, 0.6))
        c0, c1 = rng.random(3) * 0.6 + 0.2, rng.random(3) * 0.6 + 0.2
        s0, s1 = 10.0 ** rng.uniform(-2.0, -0.8, 2)
        col = np.concatenate([c0 + rng.standard_normal((n1, 3)) * s0, c1 + rng.standard_normal((n - n1, 3)) * s1]).astype(np.float32)
        col = col[rng.permutation(n)]
        q = _q(rng, n)
        _, _, tr = outlier_face(col, q, 2)
        if tr[0] == EXIT_TEN_ROUNDS and tr[3]:
            out.append((col, q, "noconv"))
            if len(out) == want:
                break
    return out


def _kept(col, q):
    return int(np.count_nonzero(outlier_face(col, q, 2)[1]))


def _fam_threshold_pairs(rng, want=104):
    """pairs of faces that differ in one float32 ulp of one colour and fall on either side of a decision: one colour of a 20-point
    cluster (sigma 0.04) is moved along a random direction by an offset bisected in float32 between 0 and 1 until two adjacent floats
    give different numbers of infos kept under clamping.  Returns the faces, members of pair k at 2 k and 2 k + 1."""
    out = []
    while len(out) < 2 * want:
        col = _cluster(rng, 20, 0.04); q = _q(rng, 20)
        d = rng.standard_normal(3); d = (d / np.linalg.norm(d)).astype(np.float32)
        base = col[0].copy()
        def face(t):
            c = col.copy(); c[0] = base + np.float32(t) * d
            return c
        lo, hi = np.float32(0.0), np.float32(1.0)
        k0 = _kept(face(lo), q)
        if _kept(face(hi), q) == k0:
            continue
        while np.nextafter(lo, np.float32(2.0)) != hi:
            mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            if _kept(face(mid), q) == k0:
                lo = mid
            else:
                hi = mid
        out += [(face(lo), q, "pair"), (face(hi), q, "pair")]
    return out


def _fam_underflow(rng, count=160):
    """clusters whose covariance stays above 5e-4 (sigma 0.04) and one outlier at a squared Mahalanobis distance swept over 780..1120:
    damping multiplies its quality by exp(-0.1 d^2), which crosses the float denormal range (d^2 in 873..1033) down to exact zero"""
    out = []
    for k in range(count):
        n = 20
        col = _cluster(rng, n, 0.04).astype(np.float64)
        mu, cov = col[1:].mean(0), np.cov(col[1:].T)
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        d2 = 780.0 + 340.0 * (k + rng.random()) / count
        col[0] = mu + u * np.sqrt(d2 / (u @ np.linalg.solve(cov, u)))
        out.append((col.astype(np.float32), _q(rng, n), "underflow"))
    return out


def non_finite_faces(rng):
    out = []
    for n in (5, 12, 21):
        for what in ("nan_channel", "inf_channel", "ninf_channel", "all_nan", "nan_last", "nan_first"):
            col = _cluster(rng, n, 0.05, 1 if n > 6 else 0)
            if what == "nan_channel":
                col[n // 2, 1] = np.nan
            elif what == "inf_channel":
                col[n // 2, 2] = np.inf
            elif what == "ninf_channel":
                col[1, 0] = -np.inf
            elif what == "all_nan":
                col[:] = np.nan
            elif what == "nan_last":
                col[-1] = np.nan
            else:
                col[0] = np.nan
            out.append((col, _q(rng, n), "nonfinite"))
    return out


def _fam_fill(rng, count, kmax=40):
    """random clusters with outliers, columns 0..kmax: what a scene produces"""
    out = []
    for _ in range(count):
        n = int(rng.integers(0, kmax + 1))
        out.append((_cluster(rng, n, 10.0 ** rng.uniform(-2.0, -1.0), int(rng.integers(0, n // 5 + 1)) if n >= 5 else 0), _q(rng, n), "fill"))
    return out


def _outlier_cases():
    rng = np.random.default_rng(20240)
    pairs = _fam_threshold_pairs(rng)
    faces = (_fam_lengths(rng) + _fam_zero_covariance(rng) + rank_deficient_faces(rng) + _fam_few_inliers(rng) + _fam_no_convergence(rng)
             + _fam_underflow(rng) + non_finite_faces(rng) + _fam_fill(rng, 200))
    n_other = len(faces)
    faces = faces + pairs
    for name, extra in (("outlier_mix_lds", []), ("outlier_mix_global", [(_cluster(rng, 90, 0.05, 9), _q(rng, 90), "long")])):
        c = _pack(name, faces + extra, np.random.default_rng(7), outlier=True)
        pos = np.argsort(c.perm)                             # where each face went
        c.info["pairs"] = np.stack([pos[n_other:n_other + len(pairs):2], pos[n_other + 1:n_other + len(pairs):2]], axis=1)
        yield c


def _handover_cases():
    """the same 500 faces and one more of LDS_MAX_COLUMN (the LDS-staged kernel), LDS_MAX_COLUMN + 1 and 300 infos (the global-memory
    kernel): the extra face is the last one, the shared faces are faces 0..499 of every call"""
    rng = np.random.default_rng(31)
    # 24 faces of three infos (returned untouched: fewer than 4) hold 72 qualities of exactly 1.0, the maximum: more than 0.5 % of
    # every call's infos, so no bin's test fires and the percentile IS the maximum in all three calls and modes -- the shared
    # faces' costs, 1 - q, then have to agree between the calls bit for bit
    pin = [(_cluster(rng, 3, 0.05), np.ones(3, np.float32), "pin") for _ in range(24)]
    shared = _fam_fill(rng, 436) + rank_deficient_faces(rng, 20) + _fam_underflow(rng, 20) + pin
    shared = [shared[i] for i in rng.permutation(len(shared))]
    seed = int(rng.integers(1 << 30))
    for n in (LDS_MAX_COLUMN, LDS_MAX_COLUMN + 1, 300):
        extra = (_cluster(np.random.default_rng(n), n, 0.05, n // 8), _q(np.random.default_rng(n + 1), n), "extra")
        yield _pack("handover_%d" % n, shared + [extra], np.random.default_rng(seed), n_views=300, interleave=False, outlier=True, info={"shared": 500})


def _face_count_cases():
    for nf in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        rng = np.random.default_rng(1000 + nf)
        faces = _fam_fill(rng, nf, kmax=12)
        if nf == 1:
            faces = [(_cluster(rng, 9, 0.05, 1), _q(rng, 9), "fill")]
        yield _pack("faces_%d" % nf, faces, rng, outlier=True)


def _seam_case():
    """the zero-quality erase (nonzero_count_kernel / nonzero_copy_kernel: one wave per 64 faces, the chunk streamed 64 entries at a
    time from its first entry): about 20 % zero input qualities; chunks of 64 faces whose entries are an exact multiple of 64, a chunk
    of zeros only, a chunk without zeros, columns of 65..200 entries that start on a 64-entry tile boundary of their chunk, runs of
    empty faces at the start, in the middle and at the end"""
    rng = np.random.default_rng(47)
    counts, zero_p = [], []
    def chunk(cnt, p):
        assert len(cnt) == 64
        counts.extend(cnt); zero_p.extend([p] * 64)
    def to_multiple(cnt):
        cnt = list(cnt); cnt[-1] += (-sum(cnt)) % 64
        return cnt
    chunk([0] * 64, 0.2)                                                           # empty faces at the start, past one chunk
    chunk([0] * 6 + to_multiple(rng.integers(1, 13, 58)), 0.2)
    chunk(to_multiple(rng.integers(0, 13, 64)), 1.0)                               # zeros only
    chunk(to_multiple(rng.integers(0, 13, 64)), 0.0)                               # no zeros
    chunk([65, 63, 129, 63, 200, 56, 100, 28, 128, 192] + [0] * 54, 0.2)           # starts at 0, 128, 320, 576, 704, 832 of the chunk
    chunk(to_multiple(rng.integers(0, 25, 64)), 0.2)
    chunk([64] * 3 + [0] * 30 + [1] * 31, 0.2)
    counts.extend([7, 3] + [0] * 70); zero_p.extend([0.2] * 72)                    # empty faces at the end, nf no multiple of 64
    faces = []
    for n, p in zip(counts, zero_p):
        q = _q(rng, n); q[rng.random(n) < p] = 0.0
        faces.append((_cluster(rng, n, 0.05, n // 8), q, "seam"))
    starts = np.cumsum([0] + counts)
    for f in (256, 258, 260, 262, 264, 265):                                       # the long columns do start on tile boundaries
        assert (starts[f] - starts[256]) % 64 == 0 and counts[f] >= 65
    return _pack("compaction_seams", faces, rng, n_views=256, interleave=False, outlier=True)


def _sort_case():
    rng = np.random.default_rng(53)
    faces = _fam_fill(rng, 300, kmax=30)
    order = [("asc", "desc", "shuffled")[i % 3] for i in range(300)]
    faces.append((_cluster(rng, 1000, 0.05, 100), _q(rng, 1000), "sort1000")); order.append("desc")
    return _pack("sort_orders", faces, rng, n_views=1000, interleave=False, order=order, outlier=True)


def _norm_case(name, q, rng, per_face=40):
    """qualities spread over faces of per_face infos; constant colours, so that the outlier modes leave them as they are too"""
    q = np.asarray(q, np.float32)
    q = q[rng.permutation(len(q))]
    faces = [(np.full((len(p), 3), 0.5, np.float32), p, "norm") for p in np.split(q, range(per_face, len(q), per_face))] if len(q) else []
    faces += [(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), "norm")] * 3
    return _pack(name, faces, rng, n_views=per_face, interleave=True)


def _norm_cases():
    """max / histogram / 99.5 % percentile / cost: each a call of its own (the percentile is global)"""
    rng = np.random.default_rng(61)
    f32 = np.float32
    yield _norm_case("norm_single", [0.37], rng)
    yield _norm_case("norm_all_equal", np.full(100, 0.25, f32), rng)
    yield _norm_case("norm_nnz0", [], rng)
    # float(num) / num_values == 0.995f exactly: not greater
    for n, ms in ((200, (1, 2)), (1000, (4, 5, 6)), (2000, (9, 10, 11))):
        for m in ms:
            yield _norm_case("norm_equality_%d_%d" % (n, m), np.concatenate([np.full(n - m, 1.5, f32), np.full(m, 3.0, f32)]), rng)
    # the bin whose test fires on both sides of percentile_kernel's thread seams (10 bins per thread), in bin 1 and in the last bin;
    # with 6 of 1000 at the maximum no test fires
    for k in (0, 1, 9, 10, 11, 5000, 9989, 9990, 9997, 9998):
        for m in (4, 6):
            mx = f32(0.5 + rng.random())
            yield _norm_case("norm_firing_%d_%d" % (k, m), np.concatenate([np.full(1000 - m, f32(mx * f32(k + 0.5) / f32(9999)), f32), np.full(m, mx, f32)]), rng)
    mx = f32(1.7)
    ks = np.unique(np.concatenate([[0, 1, 2, 9, 10, 11, 5000, 9989, 9990, 9997, 9998, 9999], rng.integers(0, 10000, 300)]))
    edge = (mx * ks.astype(f32) / f32(9999)).astype(f32)
    q = np.concatenate([edge, np.nextafter(edge, f32(-1.0)), np.nextafter(edge, f32(4.0)), [mx]]).astype(f32)
    yield _norm_case("norm_bin_edges", np.clip(q, 0, mx), rng)
    for mx in (1e-40, 1e-30, 1e30):
        q = (rng.random(500).astype(f32) * f32(mx)).astype(f32); q[7] = f32(mx)
        yield _norm_case("norm_max_%g" % mx, q, rng)


# the names of the cases, known without building them (a test module parametrises over them when it is collected)
CASE_NAMES = (("outlier_mix_lds", "outlier_mix_global") + tuple("handover_%d" % n for n in (LDS_MAX_COLUMN, LDS_MAX_COLUMN + 1, 300))
              + tuple("faces_%d" % n for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)) + ("compaction_seams", "sort_orders")
              + ("norm_single", "norm_all_equal", "norm_nnz0") + tuple("norm_equality_%d_%d" % (n, m) for n, ms in ((200, (1, 2)), (1000, (4, 5, 6)), (2000, (9, 10, 11))) for m in ms)
              + tuple("norm_firing_%d_%d" % (k, m) for k in (0, 1, 9, 10, 11, 5000, 9989, 9990, 9997, 9998) for m in (4, 6))
              + ("norm_bin_edges", "norm_max_1e-40", "norm_max_1e-30", "norm_max_1e+30"))
OUTLIER_CASE_NAMES = CASE_NAMES[:17]


@functools.lru_cache(maxsize=None)
def _all_cases():
    out = list(_outlier_cases()) + list(_handover_cases()) + list(_face_count_cases()) + [_seam_case(), _sort_case()] + list(_norm_cases())
    assert tuple(c.name for c in out) == CASE_NAMES and tuple(c.name for c in out if c.outlier) == OUTLIER_CASE_NAMES
    return tuple(out)


def postprocess_cases():
    """the named, seeded cases: each a complete input of one mvs_postprocess_face_infos call"""
    return _all_cases()


def get_case(name):
    return next(c for c in _all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference_of(name, mode):
    """postprocess_reference_traced of a case, computed once and shared (treat as read-only)"""
    out = postprocess_reference_traced(*get_case(name).args(), mode)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
