// patch_model.cpp -- CPU model of row f6 (DESIGN.md section 4 "Texture patches"): the texture patches of the labelled faces and
// TexturePatch::adjust_colors, restated SEQUENTIALLY -- candidates one after another with their own lists and texture coordinates,
// the merge loop appending and shifting them, adjust_colors face after face in list order with the masks it reads back as it goes --
// so that the order-free rule the device uses (last inside face, else first near face) is tested, not assumed.  Single-threaded,
// fp32 without contraction.  Built by patch_model.py with g++ -O2 -mfma -ffp-contract=off -fno-fast-math.  Test infrastructure:
// nothing of the product references it.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace {

struct View { float K[9]; float w2c[12]; int w, h; const uint8_t* rgb; };

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

// counters that show what the inputs exercised (tests assert they are non-zero on the crafted set)
enum { N_ABSORBED = 0, N_INSIDE_TWICE, N_NEAR_THEN_INSIDE, N_DEGENERATE, N_FRAME_NEG, N_MAGENTA_NEAR, N_MAGENTA_INSIDE, N_MAGENTA, N_CLAMPED, N_CHAIN, N_ABSORBER_LATER, N_EQUAL_BOXES,
       N_COUNTERS };

struct Tri {
    float v1x, v1y, v2x, v2y, v3x, v3y, detT, min_x, min_y, max_x, max_y;
    Tri(const float* t) : v1x(t[0]), v1y(t[1]), v2x(t[2]), v2y(t[3]), v3x(t[4]), v3y(t[5]) {
        const float T0 = v1x - v3x, T1 = v2x - v3x, T2 = v1y - v3y, T3 = v2y - v3y;
        detT = T0 * T3 - T2 * T1;
        min_x = std::min(v1x, std::min(v2x, v3x)); min_y = std::min(v1y, std::min(v2y, v3y));
        max_x = std::max(v1x, std::max(v2x, v3x)); max_y = std::max(v1y, std::max(v2y, v3y));
    }
    float area() const {
        const float ux = v2x - v1x, uy = v2y - v1y, vx = v3x - v1x, vy = v3y - v1y;
        return 0.5f * std::fabs(ux * vy - uy * vx);
    }
    void bary(float x, float y, float* b) const {
        const float alpha = ((v2y - v3y) * (x - v3x) + (v3x - v2x) * (y - v3y)) / detT;
        const float beta = ((v3y - v1y) * (x - v3x) + (v1x - v3x) * (y - v3y)) / detT;
        b[0] = alpha; b[1] = beta; b[2] = 1.0f - alpha - beta;
    }
};
float norm2(float dx, float dy) { return std::sqrt(dx * dx + dy * dy); }
float interpolate(float v1, float v2, float v3, float w1, float w2, float w3) { return (v1 * w1 + v2 * w2) + v3 * w3; }

// TexturePatch::adjust_colors on one patch: image [3 w h] in place, validity / blending [w h] (blending zero on entry, as a fresh
// patch has it), texcoords [6 n], adjust [9 n] (corner-major, channel-minor)
void adjust_colors(int w, int h, float* image, uint32_t n, const float* texcoords, const float* adjust, uint8_t* validity, uint8_t* blending,
                   uint64_t* cnt) {
    const float sqrt_2 = (float)std::sqrt(2.0);
    const size_t npx = (size_t)w * h;
    std::fill(validity, validity + npx, (uint8_t)0);
    std::vector<float> iadj(3 * npx, 0.0f);
    for (uint32_t i = 0; i < n; ++i) {
        const float* tc = texcoords + 6 * (size_t)i;
        const float* av = adjust + 9 * (size_t)i;
        const Tri tri(tc);
        const float area = tri.area();
        if (area < FLT_EPSILON) { ++cnt[N_DEGENERATE]; continue; }
        int min_x = (int)std::floor(tri.min_x) - 1, min_y = (int)std::floor(tri.min_y) - 1;
        int max_x = (int)std::ceil(tri.max_x) + 1, max_y = (int)std::ceil(tri.max_y) + 1;
        if (min_x < 0 || min_y < 0 || max_x > w || max_y > h) {   // upstream asserts; never on frames built by item 1
            ++cnt[N_CLAMPED];
            min_x = std::max(min_x, 0); min_y = std::max(min_y, 0); max_x = std::min(max_x, w); max_y = std::min(max_y, h);
        }
        for (int y = min_y; y < max_y; ++y)
            for (int x = min_x; x < max_x; ++x) {
                float b[3];
                tri.bary((float)x, (float)y, b);
                float mn = b[0]; if (b[1] < mn) mn = b[1]; if (b[2] < mn) mn = b[2];
                const size_t px = (size_t)y * w + x;
                if (mn >= 0.0f) {
                    if (validity[px] == 255) ++cnt[blending[px] == 255 ? N_INSIDE_TWICE : N_NEAR_THEN_INSIDE];
                    for (int c = 0; c < 3; ++c) iadj[3 * px + c] = interpolate(av[c], av[3 + c], av[6 + c], b[0], b[1], b[2]);
                    validity[px] = 255; blending[px] = 255;
                } else {
                    if (validity[px] == 255) continue;
                    const float ha = 2.0f * -b[0] * area / norm2(tri.v2x - tri.v3x, tri.v2y - tri.v3y);
                    const float hb = 2.0f * -b[1] * area / norm2(tri.v1x - tri.v3x, tri.v1y - tri.v3y);
                    const float hc = 2.0f * -b[2] * area / norm2(tri.v1x - tri.v2x, tri.v1y - tri.v2y);
                    if (ha > sqrt_2 || hb > sqrt_2 || hc > sqrt_2) continue;
                    for (int c = 0; c < 3; ++c) iadj[3 * px + c] = interpolate(av[c], av[3 + c], av[6 + c], b[0], b[1], b[2]);
                    validity[px] = 255; blending[px] = 64;
                }
            }
    }
    for (size_t i = 0; i < npx; ++i) {
        if (validity[i] != 0) { for (int c = 0; c < 3; ++c) image[3 * i + c] += iadj[3 * i + c]; }
        else { image[3 * i] = 0.0f; image[3 * i + 1] = 0.0f; image[3 * i + 2] = 0.0f; }
    }
}

struct Model {
    int status = 0;   // 0 ok, 4 labeling
    std::vector<uint32_t> label, face_ptr, faces; std::vector<int32_t> box; std::vector<float> texcoords, image;
    std::vector<uint64_t> pix_ptr; std::vector<uint8_t> validity, blending;
    uint64_t stats[7] = {0};   // patches, merged, listed faces, degenerate faces, pixels, valid pixels, near-only pixels
    uint64_t cnt[N_COUNTERS] = {0};
};

struct Cand { std::vector<uint32_t> faces; std::vector<float> texcoords; int min_x, min_y, max_x, max_y; uint32_t label; bool alive = true; uint32_t absorbed = 0; };

}  // namespace

extern "C" {

// corner_adjust: [9 n_faces] or null (zeros)
void* patch_model_run(uint32_t n_verts, const float* verts, uint32_t n_faces, const uint32_t* faces, uint32_t n_views, const float* K,
                      const float* w2c, const int32_t* wh, const uint8_t* const* rgb, const uint32_t* adj_ptr, const uint32_t* adj,
                      const uint32_t* labels, const float* corner_adjust) {
    Model* M = new Model();
    std::vector<View> views(n_views);
    for (uint32_t j = 0; j < n_views; ++j) {
        memcpy(views[j].K, K + 9 * j, 9 * sizeof(float)); memcpy(views[j].w2c, w2c + 12 * j, 12 * sizeof(float));
        views[j].w = wh[2 * j]; views[j].h = wh[2 * j + 1]; views[j].rgb = rgb[j];
    }
    const uint32_t F = n_faces;
    (void)n_verts;
    for (uint32_t f = 0; f < F; ++f) if (labels[f] > n_views) { M->status = 4; return M; }
    std::vector<uint32_t> used(F, 0);
    M->face_ptr.push_back(0); M->pix_ptr.push_back(0);
    for (uint32_t L = 1; L <= n_views; ++L) {
        const View& vw = views[L - 1];
        // the label's candidates: components in ascending smallest face, BFS queue order (mvs_ctx_get_subgraphs); generate_candidate
        std::vector<Cand> cands;
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
            int mnx = vw.w, mny = vw.h, mxx = 0, mxy = 0;
            for (uint32_t f : c.faces)
                for (int k = 0; k < 3; ++k) {
                    float px, py; pixel_coords(vw, verts + 3 * (size_t)faces[3 * f + k], px, py);
                    c.texcoords.push_back(px); c.texcoords.push_back(py);
                    const float fx = std::floor(px), fy = std::floor(py), cx = std::ceil(px), cy = std::ceil(py);
                    if (!(fx >= 0.0f && fy >= 0.0f && cx <= (float)(vw.w - 1) && cy <= (float)(vw.h - 1))) { M->status = 4; return M; }
                    mnx = std::min(mnx, (int)fx); mny = std::min(mny, (int)fy); mxx = std::max(mxx, (int)cx); mxy = std::max(mxy, (int)cy);
                }
            c.min_x = mnx - 1; c.min_y = mny - 1; c.max_x = mxx; c.max_y = mxy;
            const float fmx = (float)c.min_x, fmy = (float)c.min_y;
            for (size_t i = 0; i < c.texcoords.size(); i += 2) { c.texcoords[i] = c.texcoords[i] - fmx; c.texcoords[i + 1] = c.texcoords[i + 1] - fmy; }
            cands.push_back(std::move(c));
        }
        // the merge loop: lists appended, texture coordinates shifted by the difference of the frames, boxes never grown
        for (size_t i = 0; i < cands.size(); ++i) {
            if (!cands[i].alive) continue;
            for (size_t j = 0; j < cands.size(); ++j) {
                Cand& a = cands[i]; Cand& s = cands[j];
                if (j == i || !s.alive) continue;
                if (!(s.min_x >= a.min_x && s.max_x <= a.max_x && s.min_y >= a.min_y && s.max_y <= a.max_y)) continue;
                a.faces.insert(a.faces.end(), s.faces.begin(), s.faces.end());
                const float ox = (float)(s.min_x - a.min_x), oy = (float)(s.min_y - a.min_y);
                for (size_t t = 0; t < s.texcoords.size(); t += 2) { a.texcoords.push_back(s.texcoords[t] + ox); a.texcoords.push_back(s.texcoords[t + 1] + oy); }
                s.alive = false; ++M->stats[1]; ++M->cnt[N_ABSORBED];
                if (s.absorbed) ++M->cnt[N_CHAIN];                    // its list already holds other candidates' faces and offsets
                if (j < i) ++M->cnt[N_ABSORBER_LATER];
                if (s.min_x == a.min_x && s.max_x == a.max_x && s.min_y == a.min_y && s.max_y == a.max_y) ++M->cnt[N_EQUAL_BOXES];
                ++a.absorbed;
            }
        }
        // every survivor becomes a patch: crop + byte_to_float_image, then adjust_colors
        for (const Cand& c : cands) {
            if (!c.alive) continue;
            const int w = c.max_x - c.min_x + 2, h = c.max_y - c.min_y + 2;
            const size_t npx = (size_t)w * h, p0 = M->validity.size();
            M->label.push_back(c.label);
            M->box.push_back(c.min_x); M->box.push_back(c.min_y); M->box.push_back(w); M->box.push_back(h);
            if (c.min_x < 0 || c.min_y < 0) ++M->cnt[N_FRAME_NEG];
            M->faces.insert(M->faces.end(), c.faces.begin(), c.faces.end());
            M->texcoords.insert(M->texcoords.end(), c.texcoords.begin(), c.texcoords.end());
            M->face_ptr.push_back((uint32_t)M->faces.size());
            M->image.resize(3 * (p0 + npx)); M->validity.resize(p0 + npx, 0); M->blending.resize(p0 + npx, 0);
            std::vector<uint8_t> magenta(npx, 0);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const int vx = c.min_x + x, vy = c.min_y + y;
                    float* px = M->image.data() + 3 * (p0 + (size_t)y * w + x);
                    if (vx < 0 || vy < 0 || vx >= vw.w || vy >= vw.h) { px[0] = 255.0f / 255.0f; px[1] = 0.0f; px[2] = 255.0f / 255.0f; magenta[(size_t)y * w + x] = 1; ++M->cnt[N_MAGENTA]; }
                    else for (int ch = 0; ch < 3; ++ch) px[ch] = (float)vw.rgb[((size_t)vy * vw.w + vx) * 3 + ch] / 255.0f;
                }
            std::vector<float> av(9 * c.faces.size(), 0.0f);
            if (corner_adjust) for (size_t i = 0; i < c.faces.size(); ++i) memcpy(av.data() + 9 * i, corner_adjust + 9 * (size_t)c.faces[i], 9 * sizeof(float));
            adjust_colors(w, h, M->image.data() + 3 * p0, (uint32_t)c.faces.size(), c.texcoords.data(), av.data(), M->validity.data() + p0,
                          M->blending.data() + p0, M->cnt);
            for (size_t i = 0; i < npx; ++i) {
                if (M->validity[p0 + i]) { ++M->stats[5]; if (magenta[i]) ++M->cnt[M->blending[p0 + i] == 255 ? N_MAGENTA_INSIDE : N_MAGENTA_NEAR]; }
                if (M->blending[p0 + i] == 64) ++M->stats[6];
            }
            M->pix_ptr.push_back((uint64_t)M->validity.size());
        }
    }
    M->stats[0] = M->label.size(); M->stats[2] = M->faces.size(); M->stats[3] = M->cnt[N_DEGENERATE]; M->stats[4] = M->validity.size();
    return M;
}

// adjust_colors alone (the pins): image [3 w h] in place, validity / blending [w h] out
void patch_model_adjust_colors(int32_t w, int32_t h, float* image, uint32_t n, const float* texcoords, const float* adjust, uint8_t* validity,
                               uint8_t* blending, uint64_t* counters) {
    uint64_t cnt[N_COUNTERS] = {0};
    std::fill(blending, blending + (size_t)w * h, (uint8_t)0);
    adjust_colors(w, h, image, n, texcoords, adjust, validity, blending, cnt);
    if (counters) memcpy(counters, cnt, sizeof(cnt));
}

int patch_model_status(void* h) { return ((Model*)h)->status; }
void patch_model_stats(void* h, uint64_t* stats, uint64_t* counters) {
    const Model* M = (const Model*)h;
    memcpy(stats, M->stats, sizeof(M->stats)); memcpy(counters, M->cnt, sizeof(M->cnt));
}
// name -> (pointer, element count, element size)
const void* patch_model_array(void* h, const char* name, uint64_t* n) {
    Model* M = (Model*)h;
    const std::string s(name);
#define ARR(NAME) if (s == #NAME) { *n = M->NAME.size(); return M->NAME.data(); }
    ARR(label) ARR(box) ARR(face_ptr) ARR(faces) ARR(texcoords) ARR(pix_ptr) ARR(image) ARR(validity) ARR(blending)
#undef ARR
    *n = 0; return nullptr;
}
void patch_model_free(void* h) { delete (Model*)h; }

}  // extern "C"
