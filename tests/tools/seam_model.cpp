// seam_model.cpp -- CPU model of global seam leveling (row f5, DESIGN.md section 4 "Global seam leveling"): items 1-9 of the
// definition restated in their order, single-threaded, fp32 without contraction.  Built by the tests' fixture (seam_model.py) with
// g++ -O2 -mfma -ffp-contract=off -fno-fast-math.  Test infrastructure: nothing of the product references it.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace {

struct View { float K[9]; float w2c[12]; int w, h; const uint8_t* rgb; };

struct Model {
    int status = 0;   // 0 ok, 4 labeling
    std::vector<uint32_t> x_ptr, x_label, ring_ptr, ring;
    std::vector<uint32_t> a_col;      // 2 per A row: x index of (v, l1), (v, l2)
    std::vector<float> b;             // 3 per A row
    std::vector<uint32_t> lhs_ptr, lhs_col; std::vector<float> lhs_val;   // full symmetric rows, columns ascending
    std::vector<float> rhs;           // 3 per x row
    std::vector<float> x_raw, x_adjust, corner_adjust;   // 3 per x row, 3 per x row, 9 per face
    std::vector<uint32_t> patch_label, face_patch;
    uint64_t stats[8] = {0};          // patches, merged, x_rows, a_rows, gamma_rows, lower nnz, seam edges, samples
    uint32_t iters[3] = {0, 0, 0}; float err[3] = {0, 0, 0};
};

void pixel_coords(const View& v, const float* p, float& px, float& py) {
    const float* m = v.w2c;
    const float c0 = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + 1.0f * m[3];
    const float c1 = ((m[4] * p[0] + m[5] * p[1]) + m[6] * p[2]) + 1.0f * m[7];
    const float c2 = ((m[8] * p[0] + m[9] * p[1]) + m[10] * p[2]) + 1.0f * m[11];
    const float* k = v.K;
    const float q0 = (k[0] * c0 + k[1] * c1) + k[2] * c2;
    const float q1 = (k[3] * c0 + k[4] * c1) + k[5] * c2;
    const float q2 = (k[6] * c0 + k[7] * c1) + k[8] * c2;
    px = q0 / q2 - 0.5f; py = q1 / q2 - 0.5f;
}

// the fixed two-level tree of every dot product and sum (item 8): 256-element tiles, NB = min(1024, tiles) blocks; thread t of block
// b adds elements tile * 256 + t for tiles b, b + NB, ... in order, the block halves (t += t + s, s = 128 .. 1); level two does the
// same with the NB block partials in one block
float tree_sum(const std::vector<float>& v) {
    const size_t n = v.size();
    if (n == 0) return 0.0f;
    const size_t T = (n + 255) / 256, NB = std::min<size_t>(1024, T);
    std::vector<float> part(NB);
    float acc[256];
    for (size_t blk = 0; blk < NB; ++blk) {
        for (int t = 0; t < 256; ++t) {
            float a = 0.0f;
            for (size_t tile = blk; tile < T; tile += NB) { const size_t i = tile * 256 + t; if (i < n) a = a + v[i]; }
            acc[t] = a;
        }
        for (int s = 128; s >= 1; s >>= 1) for (int t = 0; t < s; ++t) acc[t] = acc[t] + acc[t + s];
        part[blk] = acc[0];
    }
    for (int t = 0; t < 256; ++t) { float a = 0.0f; for (size_t j = t; j < NB; j += 256) a = a + part[j]; acc[t] = a; }
    for (int s = 128; s >= 1; s >>= 1) for (int t = 0; t < s; ++t) acc[t] = acc[t] + acc[t + s];
    return acc[0];
}

struct Patch { int min_x, min_y, max_x, max_y; uint32_t label; };

}  // namespace

extern "C" {

void* seam_model_run(uint32_t n_verts, const float* verts, uint32_t n_faces, const uint32_t* faces, uint32_t n_views, const float* K,
                     const float* w2c, const int32_t* wh, const uint8_t* const* rgb, const uint32_t* adj_ptr, const uint32_t* adj,
                     const uint32_t* labels, float tol, uint32_t max_iters, float lambda) {
    Model* M = new Model();
    std::vector<View> views(n_views);
    for (uint32_t j = 0; j < n_views; ++j) {
        memcpy(views[j].K, K + 9 * j, 9 * sizeof(float)); memcpy(views[j].w2c, w2c + 12 * j, 12 * sizeof(float));
        views[j].w = wh[2 * j]; views[j].h = wh[2 * j + 1]; views[j].rgb = rgb[j];
    }
    const uint32_t NV = n_verts, F = n_faces;
    for (uint32_t f = 0; f < F; ++f) if (labels[f] > n_views) { M->status = 4; return M; }
    // 1. faces of every vertex (ascending, a repeated corner once) and the vertex rows
    std::vector<std::vector<uint32_t>> vf(NV);
    for (uint32_t f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = faces[3 * f + k];
            bool dup = false;
            for (int k2 = 0; k2 < k; ++k2) dup = dup || faces[3 * f + k2] == v;
            if (!dup) vf[v].push_back(f);
        }
    M->x_ptr.assign(NV + 1, 0);
    std::vector<std::vector<uint32_t>> vlab(NV);
    for (uint32_t v = 0; v < NV; ++v) {
        for (uint32_t f : vf[v]) if (labels[f]) vlab[v].push_back(labels[f]);
        std::sort(vlab[v].begin(), vlab[v].end());
        vlab[v].erase(std::unique(vlab[v].begin(), vlab[v].end()), vlab[v].end());
        M->x_ptr[v + 1] = M->x_ptr[v] + (uint32_t)vlab[v].size();
        for (uint32_t l : vlab[v]) M->x_label.push_back(l);
    }
    const uint32_t XR = M->x_ptr[NV];
    auto xrow = [&](uint32_t v, uint32_t l) -> int64_t {
        for (uint32_t i = M->x_ptr[v]; i < M->x_ptr[v + 1]; ++i) if (M->x_label[i] == l) return i;
        return -1;
    };
    // 2. ring: distinct other vertices of the incident faces, ascending
    M->ring_ptr.assign(NV + 1, 0);
    std::vector<std::vector<uint32_t>> rings(NV);
    for (uint32_t v = 0; v < NV; ++v) {
        for (uint32_t f : vf[v]) for (int k = 0; k < 3; ++k) if (faces[3 * f + k] != v) rings[v].push_back(faces[3 * f + k]);
        std::sort(rings[v].begin(), rings[v].end());
        rings[v].erase(std::unique(rings[v].begin(), rings[v].end()), rings[v].end());
        M->ring_ptr[v + 1] = M->ring_ptr[v] + (uint32_t)rings[v].size();
        M->ring.insert(M->ring.end(), rings[v].begin(), rings[v].end());
    }
    auto edge_faces = [&](uint32_t v, uint32_t u) {
        std::vector<uint32_t> out;
        for (uint32_t f : vf[v]) if (std::find(vf[u].begin(), vf[u].end(), f) != vf[u].end()) out.push_back(f);
        return out;
    };
    // 3. patches: components per label (ascending smallest face, BFS queue order), candidate boxes, merges
    std::vector<uint32_t> used(F, 0);
    struct Cand { std::vector<uint32_t> faces; int min_x, min_y, max_x, max_y; uint32_t label; int parent = -1; uint32_t off = 0, len = 0; bool alive = true; };
    std::vector<Cand> cands;
    std::vector<std::vector<float>> pc(F);   // 6 per face: the corners' pixel coordinates in the face's view
    for (uint32_t L = 1; L <= n_views; ++L) {
        const size_t c0 = cands.size();
        for (uint32_t s = 0; s < F; ++s) {
            if (labels[s] != L || used[s]) continue;
            Cand c; c.label = L;
            c.faces.push_back(s); used[s] = 1;
            for (size_t q = 0; q < c.faces.size(); ++q) {
                const uint32_t u = c.faces[q];
                for (uint32_t e = adj_ptr[u]; e < adj_ptr[u + 1]; ++e) {
                    const uint32_t w = adj[e];
                    if (labels[w] == L && !used[w]) { used[w] = 1; c.faces.push_back(w); }
                }
            }
            const View& vw = views[L - 1];
            int mnx = vw.w, mny = vw.h, mxx = 0, mxy = 0;
            for (uint32_t f : c.faces) {
                pc[f].resize(6);
                for (int k = 0; k < 3; ++k) {
                    float px, py; pixel_coords(vw, verts + 3 * (size_t)faces[3 * f + k], px, py);
                    pc[f][2 * k] = px; pc[f][2 * k + 1] = py;
                    const float fx = std::floor(px), fy = std::floor(py), cx = std::ceil(px), cy = std::ceil(py);
                    if (!(fx >= 0.0f && fy >= 0.0f && cx <= (float)(vw.w - 1) && cy <= (float)(vw.h - 1))) { M->status = 4; return M; }
                    mnx = std::min(mnx, (int)fx); mny = std::min(mny, (int)fy); mxx = std::max(mxx, (int)cx); mxy = std::max(mxy, (int)cy);
                }
            }
            c.min_x = mnx - 1; c.min_y = mny - 1; c.max_x = mxx; c.max_y = mxy;
            c.len = (uint32_t)c.faces.size();
            cands.push_back(std::move(c));
        }
        const size_t c1 = cands.size();
        for (size_t i = c0; i < c1; ++i) {
            if (!cands[i].alive) continue;
            for (size_t j = c0; j < c1; ++j) {
                Cand& a = cands[i]; Cand& s = cands[j];
                if (j == i || !s.alive) continue;
                if (s.min_x >= a.min_x && s.max_x <= a.max_x && s.min_y >= a.min_y && s.max_y <= a.max_y) {
                    s.parent = (int)i; s.off = a.len; a.len += s.len; s.alive = false; ++M->stats[1];
                }
            }
        }
    }
    std::vector<uint32_t> cand_pid(cands.size()), cand_pos(cands.size());
    std::vector<Patch> patches;
    for (size_t c = 0; c < cands.size(); ++c)
        if (cands[c].alive) { cand_pid[c] = (uint32_t)patches.size(); patches.push_back(Patch{cands[c].min_x, cands[c].min_y, cands[c].max_x, cands[c].max_y, cands[c].label}); }
    for (size_t c = 0; c < cands.size(); ++c) {
        size_t r = c; uint32_t pos = 0;
        while (cands[r].parent >= 0) { pos += cands[r].off; r = (size_t)cands[r].parent; }
        cand_pid[c] = cand_pid[r]; cand_pos[c] = pos;
    }
    M->stats[0] = patches.size();
    for (const Patch& p : patches) M->patch_label.push_back(p.label);
    M->face_patch.assign(F, 0xFFFFFFFFu);
    std::vector<uint32_t> fpos(F, 0), fcand(F, 0);
    for (size_t c = 0; c < cands.size(); ++c)
        for (size_t i = 0; i < cands[c].faces.size(); ++i) {
            const uint32_t f = cands[c].faces[i];
            M->face_patch[f] = cand_pid[c]; fpos[f] = cand_pos[c] + (uint32_t)i; fcand[f] = (uint32_t)c;
        }
    // 4. a vertex's projection in a patch: the first face of the patch's list holding it, through its candidate's chain of frames
    auto vproj = [&](uint32_t v, uint32_t P, float& ox, float& oy) {
        uint32_t best = 0xFFFFFFFFu, bf = 0;
        for (uint32_t f : vf[v]) if (M->face_patch[f] == P && fpos[f] < best) { best = fpos[f]; bf = f; }
        int k = 0; while (faces[3 * bf + k] != v) ++k;
        size_t c = fcand[bf];
        float x = pc[bf][2 * k] - (float)cands[c].min_x, y = pc[bf][2 * k + 1] - (float)cands[c].min_y;
        while (cands[c].parent >= 0) {
            const size_t p = (size_t)cands[c].parent;
            x = x + (float)(cands[c].min_x - cands[p].min_x); y = y + (float)(cands[c].min_y - cands[p].min_y);
            c = p;
        }
        ox = x; oy = y;
    };
    auto texel = [&](const Patch& P, int cx, int cy, int ch) -> float {
        const View& vw = views[P.label - 1];
        const int x = cx + P.min_x, y = cy + P.min_y;
        if (x < 0 || y < 0 || x >= vw.w || y >= vw.h) return ch == 1 ? 0.0f : 255.0f / 255.0f;
        return (float)vw.rgb[((size_t)y * vw.w + x) * 3 + ch] / 255.0f;
    };
    auto linear = [&](const Patch& P, float x, float y, float* out) {
        const int pw = P.max_x - P.min_x + 2, ph = P.max_y - P.min_y + 2;
        const float W1 = (float)(pw - 1), H1 = (float)(ph - 1);
        x = (x < W1) ? x : W1; x = (0.0f < x) ? x : 0.0f;
        y = (y < H1) ? y : H1; y = (0.0f < y) ? y : 0.0f;
        const int fx = (int)x, fy = (int)y;
        const int fx1 = std::min(fx + 1, pw - 1), fy1 = std::min(fy + 1, ph - 1);
        const float w1 = x - (float)fx, w0 = 1.0f - w1, w3 = y - (float)fy, w2 = 1.0f - w3;
        for (int ch = 0; ch < 3; ++ch) {
            const float v1 = texel(P, fx, fy, ch), v2 = texel(P, fx1, fy, ch), v3 = texel(P, fx, fy1, ch), v4 = texel(P, fx1, fy1, ch);
            out[ch] = ((v1 * (w0 * w2) + v2 * (w1 * w2)) + v3 * (w0 * w3)) + v4 * (w1 * w3);
        }
    };
    auto sample_edge = [&](const Patch& P, float p1x, float p1y, float p2x, float p2y, float* out) {
        const float dx = p2x - p1x, dy = p2y - p1y;
        const float nrm = std::sqrt(dx * dx + dy * dy);
        const uint32_t n = (uint32_t)(std::max(nrm, 1.0f) * 2.0f);
        float acc[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
        for (uint32_t s = 0; s < n; ++s) {
            const float fraction = (float)s / (float)(n - 1);
            const float sx = p1x + dx * fraction, sy = p1y + dy * fraction;
            float col[3]; linear(P, sx, sy, col);
            const float w = 1.0f - fraction;
            for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + col[ch] * w;
            wsum = wsum + w;
        }
        M->stats[7] += n;
        for (int ch = 0; ch < 3; ++ch) out[ch] = acc[ch] / wsum;
    };
    // 6. A rows and b
    std::vector<uint32_t> a_vert;
    for (uint32_t v = 0; v < NV; ++v) {
        const uint32_t m = (uint32_t)vlab[v].size();
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t k = j + 1; k < m; ++k) {
                const uint32_t l1 = vlab[v][j], l2 = vlab[v][k];
                std::vector<uint32_t> seam;   // adjacent vertex per seam-edge entry
                for (uint32_t u : rings[v]) {
                    const std::vector<uint32_t> ef = edge_faces(v, u);
                    for (size_t a = 0; a < ef.size(); ++a)
                        for (size_t c = a + 1; c < ef.size(); ++c) {
                            uint32_t la = labels[ef[a]], lb = labels[ef[c]];
                            if (!(la < lb)) std::swap(la, lb);
                            if (la != l1 || lb != l2) continue;
                            const float dx = verts[3 * u] - verts[3 * v], dy = verts[3 * u + 1] - verts[3 * v + 1], dz = verts[3 * u + 2] - verts[3 * v + 2];
                            const float len = std::sqrt((dx * dx + dy * dy) + dz * dz);
                            if (len == 0.0f) continue;
                            seam.push_back(u);
                        }
                }
                if (seam.empty()) continue;
                M->stats[6] += seam.size();
                float c1[3] = {0, 0, 0}, c2[3] = {0, 0, 0}, w1 = 0.0f, w2 = 0.0f;
                for (uint32_t u : seam) {
                    const float dx = verts[3 * u] - verts[3 * v], dy = verts[3 * u + 1] - verts[3 * v + 1], dz = verts[3 * u + 2] - verts[3 * v + 2];
                    const float len = std::sqrt((dx * dx + dy * dy) + dz * dz);
                    std::vector<uint32_t> ps;
                    for (uint32_t f : edge_faces(v, u)) if (labels[f] == l1 || labels[f] == l2) ps.push_back(M->face_patch[f]);
                    std::sort(ps.begin(), ps.end()); ps.erase(std::unique(ps.begin(), ps.end()), ps.end());
                    for (uint32_t P : ps) {
                        float p1x, p1y, p2x, p2y; vproj(v, P, p1x, p1y); vproj(u, P, p2x, p2y);
                        float col[3]; sample_edge(patches[P], p1x, p1y, p2x, p2y, col);
                        if (patches[P].label == l1) { for (int ch = 0; ch < 3; ++ch) c1[ch] = c1[ch] + col[ch] * len; w1 = w1 + len; }
                        else { for (int ch = 0; ch < 3; ++ch) c2[ch] = c2[ch] + col[ch] * len; w2 = w2 + len; }
                    }
                }
                M->a_col.push_back(M->x_ptr[v] + j); M->a_col.push_back(M->x_ptr[v] + k); a_vert.push_back(v);
                for (int ch = 0; ch < 3; ++ch) M->b.push_back(c2[ch] / w2 - c1[ch] / w1);
            }
    }
    const size_t AR = a_vert.size();
    // 5 + 7. Gamma and the system
    const float g = lambda * lambda;
    std::vector<uint32_t> a_ptr(NV + 1, 0);   // A rows of vertex v: [a_ptr[v], a_ptr[v + 1])
    for (size_t r = 0; r < AR; ++r) a_ptr[a_vert[r] + 1]++;
    for (uint32_t v = 0; v < NV; ++v) a_ptr[v + 1] += a_ptr[v];
    M->lhs_ptr.assign(XR + 1, 0); M->rhs.assign(3 * (size_t)XR, 0.0f);
    std::vector<float> diag(XR, 0.0f);
    uint64_t gamma_half = 0, lower = 0;
    for (uint32_t v = 0; v < NV; ++v) {
        const uint32_t m = (uint32_t)vlab[v].size();
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t row = M->x_ptr[v] + j, l = vlab[v][j];
            std::vector<std::pair<uint32_t, float>> e;
            uint32_t n = 0;
            for (uint32_t u : rings[v]) { const int64_t c = xrow(u, l); if (c >= 0) { ++n; if (u < v) e.push_back({(uint32_t)c, -g}); } }
            gamma_half += n;
            uint32_t cnt = 0;
            std::vector<char> partner(m, 0);
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (uint32_t r = a_ptr[v]; r < a_ptr[v + 1]; ++r) {
                const uint32_t ca = M->a_col[2 * r], cb = M->a_col[2 * r + 1];
                if (ca != row && cb != row) continue;
                ++cnt; partner[(ca == row ? cb : ca) - M->x_ptr[v]] = 1;
                const float coef = ca == row ? 1.0f : -1.0f;
                for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + coef * M->b[3 * r + ch];
            }
            for (int ch = 0; ch < 3; ++ch) M->rhs[3 * (size_t)row + ch] = acc[ch];
            float gs = 0.0f; for (uint32_t i = 0; i < n; ++i) gs = gs + g;
            for (uint32_t k = 0; k < m; ++k) {
                if (k == j) {
                    if (cnt && n) diag[row] = (float)cnt + gs; else if (cnt) diag[row] = (float)cnt; else if (n) diag[row] = gs;
                    if (cnt || n) e.push_back({row, diag[row]});
                } else if (partner[k]) e.push_back({M->x_ptr[v] + k, -1.0f});
            }
            for (uint32_t u : rings[v]) { const int64_t c = xrow(u, l); if (c >= 0 && u > v) e.push_back({(uint32_t)c, -g}); }
            for (auto& q : e) { M->lhs_col.push_back(q.first); M->lhs_val.push_back(q.second); if (q.first <= row) ++lower; }
            M->lhs_ptr[row + 1] = (uint32_t)M->lhs_col.size();
        }
    }
    M->stats[2] = XR; M->stats[3] = AR; M->stats[4] = gamma_half / 2; M->stats[5] = lower;
    // 8. Jacobi-preconditioned CG per channel, then the mean
    std::vector<float> invdiag(XR);
    for (uint32_t i = 0; i < XR; ++i) invdiag[i] = diag[i] != 0.0f ? 1.0f / diag[i] : 1.0f;
    M->x_raw.assign(3 * (size_t)XR, 0.0f); M->x_adjust.assign(3 * (size_t)XR, 0.0f);
    std::vector<float> tmpv(XR);
    auto dot = [&](const std::vector<float>& a, const std::vector<float>& c) { for (uint32_t i = 0; i < XR; ++i) tmpv[i] = a[i] * c[i]; return tree_sum(tmpv); };
    for (int ch = 0; ch < 3 && XR; ++ch) {
        std::vector<float> x(XR, 0.0f), r(XR), z(XR), p(XR), Ap(XR);
        for (uint32_t i = 0; i < XR; ++i) r[i] = M->rhs[3 * (size_t)i + ch];
        float rr = dot(r, r);
        const float rhs2 = rr;
        uint32_t it = 0; float err = 0.0f;
        if (rhs2 != 0.0f) {
            const float thr = std::max((tol * tol) * rhs2, FLT_MIN);
            for (uint32_t i = 0; i < XR; ++i) z[i] = invdiag[i] * r[i];
            float rz = dot(r, z);
            if (!(rr < thr) && max_iters > 0) {
                p = z;
                uint32_t k = 0;
                for (;;) {
                    for (uint32_t i = 0; i < XR; ++i) { float s = 0.0f; for (uint32_t q = M->lhs_ptr[i]; q < M->lhs_ptr[i + 1]; ++q) s = s + M->lhs_val[q] * p[M->lhs_col[q]]; Ap[i] = s; }
                    const float alpha = rz / dot(p, Ap);
                    for (uint32_t i = 0; i < XR; ++i) { x[i] = x[i] + alpha * p[i]; r[i] = r[i] - alpha * Ap[i]; z[i] = invdiag[i] * r[i]; }
                    rr = dot(r, r);
                    const float rz_new = dot(r, z);
                    if (rr < thr) break;
                    ++k;
                    if (k >= max_iters) break;
                    const float beta = rz_new / rz; rz = rz_new;
                    for (uint32_t i = 0; i < XR; ++i) p[i] = z[i] + beta * p[i];
                }
                it = k;
            }
            err = std::sqrt(rr / rhs2);
        }
        M->iters[ch] = it; M->err[ch] = err;
        const float mean = tree_sum(x) / (float)XR;
        for (uint32_t i = 0; i < XR; ++i) { M->x_raw[3 * (size_t)i + ch] = x[i]; M->x_adjust[3 * (size_t)i + ch] = x[i] - mean; }
    }
    // 9. per-corner adjustments
    M->corner_adjust.assign(9 * (size_t)F, 0.0f);
    for (uint32_t f = 0; f < F; ++f) {
        if (!labels[f]) continue;
        for (int k = 0; k < 3; ++k) {
            const int64_t row = xrow(faces[3 * f + k], labels[f]);
            for (int ch = 0; ch < 3; ++ch) M->corner_adjust[9 * (size_t)f + 3 * k + ch] = M->x_adjust[3 * (size_t)row + ch];
        }
    }
    return M;
}

int seam_model_status(void* h) { return ((Model*)h)->status; }
void seam_model_stats(void* h, uint64_t* stats, uint32_t* iters, float* err) {
    const Model* M = (const Model*)h;
    memcpy(stats, M->stats, sizeof(M->stats)); memcpy(iters, M->iters, sizeof(M->iters)); memcpy(err, M->err, sizeof(M->err));
}
// name -> (pointer, element count); elements are 4 bytes
const void* seam_model_array(void* h, const char* name, uint64_t* n) {
    Model* M = (Model*)h;
    const std::string s(name);
#define ARR(NAME) if (s == #NAME) { *n = M->NAME.size(); return M->NAME.data(); }
    ARR(x_ptr) ARR(x_label) ARR(ring_ptr) ARR(ring) ARR(a_col) ARR(b) ARR(lhs_ptr) ARR(lhs_col) ARR(lhs_val) ARR(rhs) ARR(x_raw) ARR(x_adjust)
    ARR(corner_adjust) ARR(patch_label) ARR(face_patch)
#undef ARR
    *n = 0; return nullptr;
}
void seam_model_free(void* h) { delete (Model*)h; }

}  // extern "C"
