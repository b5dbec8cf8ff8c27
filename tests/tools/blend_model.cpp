// blend_model.cpp -- CPU model of local seam leveling (row f7, DESIGN.md section 4 "Local seam leveling"): items 1-10 of the
// definition in upstream's own order and with upstream's own loops (std::map / std::set, the sequential writes, the erosion rounds),
// single-threaded, fp32 without contraction; the solve of item 9 follows the device's reduction tree.  Built by the tests' fixture
// (blend_model.py) with g++ -O2 -mfma -ffp-contract=off -fno-fast-math.  Test infrastructure: nothing of the product references it.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace {

enum { S_SEAM = 0, S_SKIPPED, S_INFOS, S_EPROJ, S_SAMPLES, S_BAD_SAMPLES, S_VWRITES, S_LWRITES, S_WRITTEN, S_OUTSIDE, S_BAD_WRITES, S_STRIP, S_FIXED,
       S_DEMOTED, S_PATCHES_LDS, S_PATCHES_GLOBAL, S_PIXELS_GLOBAL, S_ITERS_TOTAL, S_HIT_MAX, S_ITERS_MAX, S_N };
// what the crafted cases are made to contain (the tests assert each occurs)
enum { C_OVERWRITES = 0, C_ZERO_LINES, C_LABEL0_SEAMS, C_DUPLICATE_EDGES, C_VERTICES_3, C_INNER_PIXELS, C_RING_PIXELS, C_SANITIZED, C_CLAMPED_IDX, C_N };

struct Model {
    int status = 0;   // 0 ok, 4 labeling
    std::vector<float> image, after_writes; std::vector<uint8_t> validity, blending, blend_writes;
    std::vector<uint32_t> iters; std::vector<float> err;   // 3 per patch
    uint64_t stats[S_N] = {0}, counters[C_N] = {0};
    float error_max = 0.0f;
};

struct Frame { int w, h; uint64_t base; };

// mve::Image<float>::linear_at and TexturePatch::valid_pixel(Vec2f)
bool linear_at(const Frame& fr, const float* image, const uint8_t* validity, float x, float y, float* out) {
    const float width = (float)fr.w, height = (float)fr.h;
    bool valid = 0.0f <= x && x < width && 0.0f <= y && y < height;
    const float W1 = (float)(fr.w - 1), H1 = (float)(fr.h - 1);
    x = (x < W1) ? x : W1; x = (0.0f < x) ? x : 0.0f;
    y = (y < H1) ? y : H1; y = (0.0f < y) ? y : 0.0f;
    const int fx = (int)x, fy = (int)y;
    const int fx1 = std::min(fx + 1, fr.w - 1), fy1 = std::min(fy + 1, fr.h - 1);
    const float w1 = x - (float)fx, w0 = 1.0f - w1, w3 = y - (float)fy, w2 = 1.0f - w3;
    const uint64_t i1 = fr.base + (uint64_t)fy * fr.w + fx, i2 = fr.base + (uint64_t)fy * fr.w + fx1, i3 = fr.base + (uint64_t)fy1 * fr.w + fx, i4 = fr.base + (uint64_t)fy1 * fr.w + fx1;
    for (int ch = 0; ch < 3; ++ch) {
        const float v1 = image[3 * i1 + ch], v2 = image[3 * i2 + ch], v3 = image[3 * i3 + ch], v4 = image[3 * i4 + ch];
        out[ch] = ((v1 * (w0 * w2) + v2 * (w1 * w2)) + v3 * (w0 * w3)) + v4 * (w1 * w3);
    }
    if (valid)
        valid = (w0 * w2 == 0.0f || validity[i1] == 255) && (w1 * w2 == 0.0f || validity[i2] == 255) && (w0 * w3 == 0.0f || validity[i3] == 255) &&
                (w1 * w3 == 0.0f || validity[i4] == 255);
    return valid;
}

// TexturePatch::prepare_blending_mask (texture_patch.cpp:197-297), loop for loop
void prepare_blending_mask(int width, int height, const uint8_t* validity, uint8_t* blending, size_t strip_width, uint64_t* counters) {
    typedef std::vector<std::pair<int, int>> PixelVector;
    typedef std::set<std::pair<int, int>> PixelSet;
    auto at = [&](int x, int y) { return (size_t)y * width + x; };
    PixelSet valid_border_pixels;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            if (validity[at(x, y)] == 0) continue;
            if (x == 0 || x == width - 1 || y == 0 || y == height - 1) { valid_border_pixels.insert({x, y}); continue; }
            for (int j = -1; j <= 1; ++j)
                for (int i = -1; i <= 1; ++i)
                    if (validity[at(x + i, y + j)] == 0) valid_border_pixels.insert({x, y});
        }
    std::vector<uint8_t> inner_pixel(validity, validity + (size_t)width * height);
    for (size_t i = 0; i < strip_width; ++i) {
        PixelVector new_invalid_pixels(valid_border_pixels.begin(), valid_border_pixels.end());
        valid_border_pixels.clear();
        for (auto& q : new_invalid_pixels) inner_pixel[at(q.first, q.second)] = 0;
        for (auto& q : new_invalid_pixels)
            for (int j = -1; j <= 1; j++)
                for (int i2 = -1; i2 <= 1; i2++) {
                    const int nx = q.first + i2, ny = q.second + j;
                    if (0 <= nx && nx < width && 0 <= ny && ny < height && inner_pixel[at(nx, ny)] == 255) valid_border_pixels.insert({nx, ny});
                }
    }
    for (int y = 1; y < height - 1; ++y)
        for (int x = 1; x < width - 1; ++x)
            if (blending[at(x, y)] == 128) {
                const uint8_t n[] = {blending[at(x - 1, y)], blending[at(x + 1, y)], blending[at(x, y - 1)], blending[at(x, y + 1)]};
                bool valid = true;
                for (uint8_t v : n) { if (v == 255) continue; valid = false; }
                if (valid) { blending[at(x, y)] = 255; if (counters) ++counters[C_SANITIZED]; }
            }
    for (size_t i = 0; i < (size_t)width * height; ++i) if (inner_pixel[i] == 255) { blending[i] = 0; if (counters) ++counters[C_INNER_PIXELS]; }
    for (auto& q : valid_border_pixels) { blending[at(q.first, q.second)] = 128; if (counters) ++counters[C_RING_PIXELS]; }
}

// the tree of item 9: lane l of 1024 adds elements l, l + 1024, ... in order, then the lanes halve
float tree_sum(const std::vector<float>& v) {
    float acc[1024];
    for (int t = 0; t < 1024; ++t) { float a = 0.0f; for (size_t k = t; k < v.size(); k += 1024) a = a + v[k]; acc[t] = a; }
    for (int s = 512; s >= 1; s >>= 1) for (int t = 0; t < s; ++t) acc[t] = acc[t] + acc[t + s];
    return acc[0];
}

struct SolveOut { uint32_t iters[3]; float err[3]; uint64_t unknowns, fixed, demoted; };

// items 8 and 9 on one patch: mask = the prepared mask, orig = the image before the writes, x = the image after them (in / out)
void solve_patch(int w, int h, const uint8_t* mask, const float* orig, float* x, float tol, uint32_t max_iters, SolveOut& o) {
    o = SolveOut{};
    const size_t npix = (size_t)w * h;
    std::vector<uint8_t> unk(npix, 0);
    std::vector<uint32_t> list;
    for (int y = 0; y < h; ++y)
        for (int xx = 0; xx < w; ++xx) {
            const size_t j = (size_t)y * w + xx;
            if (mask[j] == 255) {
                if (xx >= 1 && y >= 1 && xx < w - 1 && y < h - 1 && mask[j - 1] != 0 && mask[j + 1] != 0 && mask[j - w] != 0 && mask[j + w] != 0) { unk[j] = 1; list.push_back((uint32_t)j); }
                else ++o.demoted;
            } else if (mask[j] == 64 || mask[j] == 128) ++o.fixed;
        }
    const size_t n = list.size();
    o.unknowns = n;
    if (!n || max_iters == 0) return;
    auto lap = [&](const float* img, size_t j, int ch) { return (((-4.0f * img[3 * j + ch] + img[3 * (j - w) + ch]) + img[3 * (j - 1) + ch]) + img[3 * (j + 1) + ch]) + img[3 * (j + w) + ch]; };
    for (int ch = 0; ch < 3; ++ch) {
        std::vector<float> p(npix, 0.0f), rhs(n), r(n), tmp(n);
        for (size_t k = 0; k < n; ++k) p[list[k]] = x[3 * (size_t)list[k] + ch];   // x0 on the unknowns, 0 on fixed pixels
        auto ap = [&](size_t j) { return (((4.0f * p[j] - p[j - w]) - p[j - 1]) - p[j + 1]) - p[j + w]; };
        for (size_t k = 0; k < n; ++k) {
            const size_t j = list[k];
            const float b = 1.0f * lap(orig, j, ch) + 0.0f * lap(x, j, ch);
            float s = -b;
            const size_t nb[4] = {j - w, j - 1, j + 1, j + w};
            for (int q = 0; q < 4; ++q) if (!unk[nb[q]]) s = s + x[3 * nb[q] + ch];
            rhs[k] = s; r[k] = s - ap(j);
        }
        for (size_t k = 0; k < n; ++k) tmp[k] = rhs[k] * rhs[k];
        const float bb = tree_sum(tmp);
        for (size_t k = 0; k < n; ++k) tmp[k] = r[k] * r[k];
        float rr = tree_sum(tmp);
        const float thr = std::max((tol * tol) * bb, FLT_MIN);
        float err = bb != 0.0f ? std::sqrt(rr / bb) : 0.0f;
        uint32_t it = 0;
        if (bb != 0.0f && !(rr < thr)) {
            float abs_new = rr;
            for (size_t k = 0; k < n; ++k) p[list[k]] = r[k];
            for (;;) {
                std::vector<float> apv(n);
                for (size_t k = 0; k < n; ++k) { apv[k] = ap(list[k]); tmp[k] = p[list[k]] * apv[k]; }
                const float alpha = abs_new / tree_sum(tmp);
                for (size_t k = 0; k < n; ++k) {
                    const size_t j = list[k];
                    x[3 * j + ch] = x[3 * j + ch] + alpha * p[j];
                    r[k] = r[k] - alpha * apv[k];
                    tmp[k] = r[k] * r[k];
                }
                rr = tree_sum(tmp);
                err = std::sqrt(rr / bb);
                if (rr < thr) break;
                ++it;
                if (it >= max_iters) break;
                const float beta = rr / abs_new; abs_new = rr;
                for (size_t k = 0; k < n; ++k) p[list[k]] = r[k] + beta * p[list[k]];
            }
        }
        o.iters[ch] = it; o.err[ch] = err;
    }
}

struct VInfo { uint32_t patch; float px, py; std::vector<uint32_t> faces; };
struct EProj { uint32_t patch; float p1x, p1y, p2x, p2y; bool operator<(const EProj& o) const { return patch < o.patch; } };

}  // namespace

extern "C" {

void* blend_model_run(uint32_t n_verts, uint32_t n_faces, const uint32_t* faces, const uint32_t* adj_ptr, const uint32_t* adj, const uint32_t* labels,
                      uint32_t NP, uint32_t n_listed, uint64_t n_pixels, const uint32_t* label, const int32_t* box, const uint32_t* face_ptr,
                      const uint32_t* pfaces, const float* texcoords, const uint64_t* pix_ptr, const float* image, const uint8_t* validity,
                      const uint8_t* blending, float tol, uint32_t max_iters, uint32_t strip_width, uint32_t lds_bytes) {
    Model* M = new Model();
    uint64_t* st = M->stats; uint64_t* cn = M->counters;
    // 1. vertex projection infos: patches ascending, list order, merged per patch (the first projection stays, faces appended)
    std::vector<std::vector<VInfo>> vinfos(n_verts);
    for (uint32_t p = 0; p < NP; ++p)
        for (uint32_t e = face_ptr[p]; e < face_ptr[p + 1]; ++e) {
            const uint32_t f = pfaces[e];
            if (f >= n_faces || labels[f] != label[p]) { M->status = 4; return M; }
            for (int k = 0; k < 3; ++k) vinfos[faces[3 * (size_t)f + k]].push_back(VInfo{p, texcoords[6 * (size_t)e + 2 * k], texcoords[6 * (size_t)e + 2 * k + 1], {f}});
        }
    for (auto& infos : vinfos) {
        std::map<uint32_t, VInfo> info_map;
        for (const VInfo& info : infos) {
            auto it = info_map.find(info.patch);
            if (it == info_map.end()) info_map[info.patch] = info; else it->second.faces.insert(it->second.faces.end(), info.faces.begin(), info.faces.end());
        }
        infos.clear();
        for (auto& kv : info_map) infos.push_back(kv.second);
        st[S_INFOS] += infos.size();
        if (infos.size() >= 3) ++cn[C_VERTICES_3];
    }
    // 2. seam edges
    std::vector<std::pair<uint32_t, uint32_t>> seam_edges;
    std::set<std::pair<uint32_t, uint32_t>> seen_edges;
    for (uint32_t node = 0; node < n_faces; ++node)
        for (uint32_t q = adj_ptr[node]; q < adj_ptr[node + 1]; ++q) {
            const uint32_t a = adj[q];
            if (node > a) continue;
            if (labels[node] == labels[a]) continue;
            std::vector<uint32_t> shared;
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) if (faces[3 * (size_t)node + i] == faces[3 * (size_t)a + j]) shared.push_back(faces[3 * (size_t)node + i]);
            if (shared.size() != 2 || shared[0] == shared[1]) { ++st[S_SKIPPED]; continue; }
            uint32_t v1 = shared[0], v2 = shared[1];
            if (v1 > v2) std::swap(v1, v2);
            if (!seen_edges.insert({v1, v2}).second) ++cn[C_DUPLICATE_EDGES];
            if (labels[node] == 0 || labels[a] == 0) ++cn[C_LABEL0_SEAMS];
            seam_edges.push_back({v1, v2});
        }
    st[S_SEAM] = seam_edges.size();
    // 3. edge projections
    std::vector<std::vector<EProj>> eproj(seam_edges.size());
    for (size_t i = 0; i < seam_edges.size(); ++i) {
        std::set<EProj> s;
        for (const VInfo& a : vinfos[seam_edges[i].first])
            for (const VInfo& b : vinfos[seam_edges[i].second]) {
                if (a.patch != b.patch) continue;
                for (uint32_t f1 : a.faces) for (uint32_t f2 : b.faces) { if (f1 != f2) continue; s.insert(EProj{a.patch, a.px, a.py, b.px, b.py}); }
            }
        eproj[i].assign(s.begin(), s.end());
        st[S_EPROJ] += eproj[i].size();
    }
    auto frame = [&](uint32_t p) { return Frame{box[4 * p + 2], box[4 * p + 3], pix_ptr[p]}; };
    // 4. edge colours and the lines
    struct Line { int x0, y0, x1, y1; size_t edge; };
    struct Pixel { int x, y; uint32_t vertex; };
    std::vector<std::vector<Line>> lines(NP);
    std::vector<std::vector<Pixel>> pixels(NP);
    std::vector<std::vector<float>> edge_colors(seam_edges.size());
    for (size_t i = 0; i < eproj.size(); ++i) {
        float max_length = 1.0f;
        for (const EProj& q : eproj[i]) { const float dx = q.p1x - q.p2x, dy = q.p1y - q.p2y; max_length = std::max(max_length, std::sqrt(dx * dx + dy * dy)); }
        const size_t n = (size_t)std::ceil(max_length * 2.0f);
        edge_colors[i].resize(3 * n);
        for (size_t j = 0; j < n; ++j) {
            const float t = (float)j / (float)(n - 1);
            float sum[3] = {0.0f, 0.0f, 0.0f}, w = 0.0f;
            for (const EProj& q : eproj[i]) {
                const float px = q.p1x * t + (1.0f - t) * q.p2x, py = q.p1y * t + (1.0f - t) * q.p2y;
                float col[3];
                if (!linear_at(frame(q.patch), image, validity, px, py, col)) ++st[S_BAD_SAMPLES];
                for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + col[ch] * 1.0f;
                w = w + 1.0f; ++st[S_SAMPLES];
            }
            for (int ch = 0; ch < 3; ++ch) edge_colors[i][3 * j + ch] = sum[ch] / w;
        }
        for (const EProj& q : eproj[i]) lines[q.patch].push_back(Line{(int)(q.p1x + 0.5f), (int)(q.p1y + 0.5f), (int)(q.p2x + 0.5f), (int)(q.p2y + 0.5f), i});
    }
    // 5. vertex colours and the vertex pixels
    std::vector<float> vertex_colors(3 * (size_t)n_verts, 0.0f);
    for (uint32_t v = 0; v < n_verts; ++v) {
        if (vinfos[v].size() <= 1) continue;
        float sum[3] = {0.0f, 0.0f, 0.0f}, w = 0.0f;
        for (const VInfo& q : vinfos[v]) {
            float col[3];
            if (!linear_at(frame(q.patch), image, validity, q.px, q.py, col)) ++st[S_BAD_SAMPLES];
            for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + col[ch] * 1.0f;
            w = w + 1.0f; ++st[S_SAMPLES];
        }
        for (int ch = 0; ch < 3; ++ch) vertex_colors[3 * (size_t)v + ch] = sum[ch] / w;
        for (const VInfo& q : vinfos[v]) pixels[q.patch].push_back(Pixel{(int)(q.px + 0.5f), (int)(q.py + 0.5f), v});
    }
    // 6 - 10. per patch
    M->image.assign(image, image + 3 * n_pixels); M->validity.assign(validity, validity + n_pixels); M->blending.assign(blending, blending + n_pixels);
    M->iters.assign(3 * (size_t)NP, 0); M->err.assign(3 * (size_t)NP, 0.0f);
    for (uint32_t p = 0; p < NP; ++p) {
        const Frame fr = frame(p);
        const size_t npix = (size_t)fr.w * fr.h;
        float* img = M->image.data() + 3 * fr.base; uint8_t* bl = M->blending.data() + fr.base; uint8_t* val = M->validity.data() + fr.base;
        std::vector<uint8_t> written(npix, 0);
        auto set_pixel = [&](int x, int y, const float* col, int counter) {
            ++st[counter];
            if (x < 0 || y < 0 || x >= fr.w || y >= fr.h) { ++st[S_OUTSIDE]; return; }
            const size_t j = (size_t)y * fr.w + x;
            if (val[j] == 0) ++st[S_BAD_WRITES];
            if (written[j]) ++cn[C_OVERWRITES]; else { written[j] = 1; ++st[S_WRITTEN]; }
            img[3 * j] = col[0]; img[3 * j + 1] = col[1]; img[3 * j + 2] = col[2]; bl[j] = 128;
        };
        for (const Pixel& q : pixels[p]) set_pixel(q.x, q.y, vertex_colors.data() + 3 * (size_t)q.vertex, S_VWRITES);
        for (const Line& ln : lines[p]) {   // draw_line
            const std::vector<float>& ec = edge_colors[ln.edge];
            const size_t n = ec.size() / 3;
            const int x0 = ln.x0, y0 = ln.y0, x1 = ln.x1, y1 = ln.y1;
            float tdx = (float)(x1 - x0), tdy = (float)(y1 - y0);
            const float length = std::sqrt(tdx * tdx + tdy * tdy);
            if (length == 0.0f) ++cn[C_ZERO_LINES];
            const int dx = std::abs(x1 - x0), dy = std::abs(y1 - y0), sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
            int err = dx - dy, x = x0, y = y0;
            while (true) {
                tdx = (float)(x1 - x); tdy = (float)(y1 - y);
                const float t = (length != 0.0f) ? std::sqrt(tdx * tdx + tdy * tdy) / length : 0.5f;
                float col[3];
                if (t < 1.0f && n > 1) {
                    size_t idx = (size_t)std::floor(t * (float)(n - 1));
                    if (idx > n - 2) { idx = n - 2; ++cn[C_CLAMPED_IDX]; }
                    for (int ch = 0; ch < 3; ++ch) col[ch] = (1.0f - t) * ec[3 * idx + ch] + t * ec[3 * (idx + 1) + ch];
                } else {
                    for (int ch = 0; ch < 3; ++ch) col[ch] = ec[3 * (n - 1) + ch];
                }
                set_pixel(x, y, col, S_LWRITES);
                if (x == x1 && y == y1) break;
                const int e2 = 2 * err;
                if (e2 > -dy) { err -= dy; x += sx; }
                if (e2 < dx) { err += dx; y += sy; }
            }
        }
        if (M->after_writes.empty()) { M->after_writes.assign(image, image + 3 * n_pixels); M->blend_writes.assign(blending, blending + n_pixels); }
        memcpy(M->after_writes.data() + 3 * fr.base, img, 3 * npix * sizeof(float)); memcpy(M->blend_writes.data() + fr.base, bl, npix);
        prepare_blending_mask(fr.w, fr.h, validity + fr.base, bl, strip_width, cn);
        SolveOut so;
        solve_patch(fr.w, fr.h, bl, image + 3 * fr.base, img, tol, max_iters, so);
        st[S_STRIP] += so.unknowns; st[S_FIXED] += so.fixed; st[S_DEMOTED] += so.demoted;
        if (so.unknowns) {
            const uint64_t need = 12ull * npix + 16ull * so.unknowns;
            if (need > std::min<uint64_t>(lds_bytes, 147456)) { ++st[S_PATCHES_GLOBAL]; st[S_PIXELS_GLOBAL] += npix; } else ++st[S_PATCHES_LDS];
        }
        bool hit = false;
        for (int ch = 0; ch < 3; ++ch) {
            M->iters[3 * (size_t)p + ch] = so.iters[ch]; M->err[3 * (size_t)p + ch] = so.err[ch];
            st[S_ITERS_TOTAL] += so.iters[ch]; st[S_ITERS_MAX] = std::max<uint64_t>(st[S_ITERS_MAX], so.iters[ch]); M->error_max = std::max(M->error_max, so.err[ch]);
            hit = hit || (max_iters > 0 && so.iters[ch] >= max_iters);
        }
        if (hit) ++st[S_HIT_MAX];
        for (size_t j = 0; j < npix; ++j) if (bl[j] == 64) val[j] = 0;
    }
    return M;
}

int blend_model_status(void* h) { return ((Model*)h)->status; }
void blend_model_stats(void* h, uint64_t* stats, uint64_t* counters, float* error_max) {
    const Model* M = (const Model*)h;
    memcpy(stats, M->stats, sizeof(M->stats)); memcpy(counters, M->counters, sizeof(M->counters)); *error_max = M->error_max;
}
// name -> (pointer, element count)
const void* blend_model_array(void* h, const char* name, uint64_t* n) {
    Model* M = (Model*)h;
    const std::string s(name);
#define ARR(NAME) if (s == #NAME) { *n = M->NAME.size(); return M->NAME.data(); }
    ARR(image) ARR(validity) ARR(blending) ARR(after_writes) ARR(blend_writes) ARR(iters) ARR(err)
#undef ARR
    *n = 0; return nullptr;
}
void blend_model_free(void* h) { delete (Model*)h; }

// upstream's prepare_blending_mask on one patch (blending in / out)
void blend_model_prepare_mask(int32_t w, int32_t h, const uint8_t* validity, uint8_t* blending, uint32_t strip_width) {
    prepare_blending_mask(w, h, validity, blending, strip_width, nullptr);
}
// items 8 - 9 on one patch alone: x = the image after the writes (in / out); out6 = iterations[3] then error[3] as bits; counts = unknowns, fixed, demoted
void blend_model_solve(int32_t w, int32_t h, const uint8_t* mask, const float* orig, float* x, float tol, uint32_t max_iters, uint32_t* iters, float* err, uint64_t* counts) {
    SolveOut so;
    solve_patch(w, h, mask, orig, x, tol, max_iters, so);
    for (int ch = 0; ch < 3; ++ch) { iters[ch] = so.iters[ch]; err[ch] = so.err[ch]; }
    counts[0] = so.unknowns; counts[1] = so.fixed; counts[2] = so.demoted;
}

}  // extern "C"
