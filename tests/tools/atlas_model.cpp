// atlas_model.cpp -- CPU model of row f8 (DESIGN.md section 4 "Texture atlases"): tex::generate_texture_atlases on a patch set, tone
// mapping `none`.  It restates upstream's loops with upstream's containers (std::list of patches and of free rectangles, std::set of
// frontier pixels, std::map of texture coordinates), so that the order-dependent wording of the definition is executable; the device
// code implements the order-free forms and is held to this model bit for bit.  float_to_byte_image is DEFINED HERE (MVE is absent).
// Test infrastructure only.  Built by atlas_model.py with g++ -O2 -mfma -ffp-contract=off -fno-fast-math.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace {

constexpr unsigned MAX_SIZE = 8192, PREF_SIZE = 4096, MIN_SIZE = 256;
enum { ST_OK = 0, ST_UNSUPPORTED = 7, ST_INTERNAL = 100 };
// counts shared with mvs_atlas_stats, in its order
enum { S_ATLASES = 0, S_256, S_512, S_1024, S_2048, S_4096, S_8192, S_PIXELS, S_VALID, S_PADDED, S_FREE_PEAK, S_MERGED, S_N };
// situations the tests ask for
enum { C_PREF_JUMP = 0, C_HALVINGS, C_BREAKS, C_BREAK_WIDEST, C_WAITS_TOO_WIDE, C_TIES, C_REFUSED_INSERTS, C_FOREIGN_FILL, C_OUTER_RING, C_WRAPPED_AREA, C_N };

struct Box { int min_x, min_y, max_x, max_y; int width() const { return max_x - min_x; } int height() const { return max_y - min_y; } int size() const { return width() * height(); } };

struct Patch { uint32_t id; int w, h; int size() const { return w * h; } };

// item 3: the guillotine bin
struct Bin {
    unsigned width, height;
    std::list<Box> rects;
    Bin(unsigned w, unsigned h) : width(w), height(h) { rects.push_back(Box{0, 0, (int)w, (int)h}); }
    bool insert(Box* r) {
        unsigned best = width * height;
        auto best_it = rects.end();
        for (auto it = rects.begin(); it != rects.end(); ++it) {
            if (r->width() <= it->width() && r->height() <= it->height()) {
                const unsigned score = it->size() - r->size();
                if (score < best) { best = score; best_it = it; }
            }
        }
        if (best_it == rects.end()) return false;
        const Box b = *best_it;
        rects.erase(best_it);
        *r = Box{b.min_x, b.min_y, b.min_x + r->width(), b.min_y + r->height()};
        const Box h_top{b.min_x, r->max_y, b.max_x, b.max_y}, h_bottom{r->max_x, b.min_y, b.max_x, r->max_y};
        const Box v_left{b.min_x, r->max_y, r->max_x, b.max_y}, v_right{r->max_x, b.min_y, b.max_x, b.max_y};
        float hr = 1.0f, vr = 1.0f;
        if (h_top.size() != 0 && h_bottom.size() != 0) hr = static_cast<float>(h_top.size()) / h_bottom.size();
        if (v_left.size() != 0 && v_right.size() != 0) vr = static_cast<float>(v_left.size()) / v_right.size();
        if (std::abs(1.0f - hr) < std::abs(1.0f - vr)) {
            if (v_left.size() != 0) rects.push_back(v_left);
            if (v_right.size() != 0) rects.push_back(v_right);
        } else {
            if (h_top.size() != 0) rects.push_back(h_top);
            if (h_bottom.size() != 0) rects.push_back(h_bottom);
        }
        return true;
    }
};

struct Model {
    int status = ST_OK;
    std::vector<uint32_t> atlas_size, patch_atlas, patch_order, face_ptr, faces, tc_ptr, texcoord_ids;
    std::vector<uint64_t> atlas_pix_ptr;
    std::vector<int32_t> patch_pos;
    std::vector<uint8_t> image;
    std::vector<float> texcoords, texcoords_merged;
    uint64_t stats[S_N] = {}, counters[C_N] = {};
    double ms_pack = 0, ms_total = 0;
};

// item 2
unsigned texture_size(const std::list<Patch>& patches, Model& M) {
    unsigned size = MAX_SIZE;
    while (true) {
        unsigned total_area = 0, max_width = 0, max_height = 0;
        const unsigned padding = size >> 7;
        unsigned long long exact_area = 0;
        bool broke = false, break_widest = false;
        for (const Patch& p : patches) {
            const unsigned width = p.w + 2 * padding, height = p.h + 2 * padding;
            const unsigned widest_before = max_width;
            max_width = std::max(max_width, width);
            max_height = std::max(max_height, height);
            const unsigned area = width * height;
            const unsigned waste = area - p.size();
            if (static_cast<double>(waste) / p.size() > 1.0) { broke = true; break_widest = &p != &patches.front() && width > widest_before; break; }
            total_area += area; exact_area += area;
        }
        if (broke) { ++M.counters[C_BREAKS]; if (break_widest) ++M.counters[C_BREAK_WIDEST]; }
        if (exact_area != total_area) ++M.counters[C_WRAPPED_AREA];
        if (!(max_width < MAX_SIZE && max_height < MAX_SIZE)) { M.status = ST_INTERNAL; return MIN_SIZE; }   // (refused before the packing starts)
        if (size > PREF_SIZE && max_width < PREF_SIZE && max_height < PREF_SIZE && total_area / (PREF_SIZE * PREF_SIZE) < 8) {
            size = PREF_SIZE; ++M.counters[C_PREF_JUMP];
            continue;
        }
        if (size <= MIN_SIZE) return MIN_SIZE;
        if (max_height < size / 2 && max_width < size / 2 && static_cast<double>(total_area) / (size * size) < 0.2) {
            size = size / 2; ++M.counters[C_HALVINGS];
            continue;
        }
        return size;
    }
}

// item 5, DEFINED HERE: mve::image::float_to_byte_image(img, 0.0f, 1.0f)
inline uint8_t float_to_byte(float x) {
    const float vmin = 0.0f, vmax = 1.0f;
    float v = std::min(vmax, std::max(vmin, x));
    v = (255.0f * (v - vmin)) / (vmax - vmin);
    return static_cast<uint8_t>(v + 0.5f);
}

struct VecLess {
    bool operator()(const std::pair<float, float>& a, const std::pair<float, float>& b) const { return a.first < b.first || (a.first == b.first && a.second < b.second); }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void run(Model& M, uint32_t NP, const int32_t* box, const uint32_t* fptr, const uint32_t* pfaces, const float* ptc, const uint64_t* pix_ptr, const float* pimage,
         const uint8_t* pvalid, bool pack_only) {
    const double t0 = now_ms();
    for (uint32_t p = 0; p < NP; ++p)
        if (box[4 * p + 2] + 128 >= (int)MAX_SIZE || box[4 * p + 3] + 128 >= (int)MAX_SIZE) { M.status = ST_UNSUPPORTED; return; }
    // item 1: popped from the back, then the stable list sort by size, descending
    std::list<Patch> patches;
    for (uint32_t k = NP; k-- > 0;) patches.push_back(Patch{k, box[4 * k + 2], box[4 * k + 3]});
    patches.sort([](const Patch& a, const Patch& b) { return a.size() > b.size(); });
    for (auto it = patches.begin(); it != patches.end(); ++it) { auto nx = std::next(it); if (nx != patches.end() && nx->size() == it->size()) ++M.counters[C_TIES]; }
    M.patch_atlas.assign(NP, 0); M.patch_pos.assign(2 * (size_t)NP, 0);
    std::vector<Box> rect_of(NP);
    std::vector<std::vector<uint32_t>> members;
    M.stats[S_FREE_PEAK] = 0;
    // item 4
    while (!patches.empty()) {
        const unsigned size = texture_size(patches, M);
        if (M.status) return;
        const unsigned padding = size >> 7;
        const uint32_t a = (uint32_t)M.atlas_size.size();
        M.atlas_size.push_back(size);
        members.emplace_back();
        Bin bin(size, size);
        M.stats[S_FREE_PEAK] = std::max<uint64_t>(M.stats[S_FREE_PEAK], 1);
        for (auto it = patches.begin(); it != patches.end();) {
            Box r{0, 0, it->w + 2 * (int)padding, it->h + 2 * (int)padding};
            if (bin.insert(&r)) {
                M.patch_atlas[it->id] = a; M.patch_pos[2 * (size_t)it->id] = r.min_x; M.patch_pos[2 * (size_t)it->id + 1] = r.min_y;
                rect_of[it->id] = r; members[a].push_back(it->id); M.patch_order.push_back(it->id);
                M.stats[S_FREE_PEAK] = std::max<uint64_t>(M.stats[S_FREE_PEAK], bin.rects.size());
                it = patches.erase(it);
            } else {
                ++M.counters[C_REFUSED_INSERTS];
                if (r.width() > (int)size || r.height() > (int)size) ++M.counters[C_WAITS_TOO_WIDE];
                ++it;
            }
        }
        if (members[a].empty()) { M.status = ST_INTERNAL; return; }   // the invariant of item 2
    }
    const uint32_t A = (uint32_t)M.atlas_size.size();
    M.stats[S_ATLASES] = A;
    M.atlas_pix_ptr.assign((size_t)A + 1, 0);
    for (uint32_t a = 0; a < A; ++a) {
        const unsigned s = M.atlas_size[a];
        M.atlas_pix_ptr[a + 1] = M.atlas_pix_ptr[a] + (uint64_t)s * s;
        ++M.stats[S_256 + (s == 256 ? 0 : s == 512 ? 1 : s == 1024 ? 2 : s == 2048 ? 3 : s == 4096 ? 4 : 5)];
    }
    M.stats[S_PIXELS] = M.atlas_pix_ptr[A];
    M.ms_pack = now_ms() - t0;
    if (pack_only) { M.ms_total = M.ms_pack; return; }
    M.image.assign(3 * (size_t)M.atlas_pix_ptr[A], 0);
    M.face_ptr.assign((size_t)A + 1, 0); M.tc_ptr.assign((size_t)A + 1, 0);
    for (uint32_t a = 0; a < A; ++a) {
        const int size = (int)M.atlas_size[a], padding = size >> 7;
        uint8_t* img = M.image.data() + 3 * (size_t)M.atlas_pix_ptr[a];
        std::vector<uint8_t> mask((size_t)size * size, 0);
        std::vector<int32_t> owner((size_t)size * size, -1), source((size_t)size * size, -1);
        std::vector<std::pair<float, float>> tcs;
        // item 5 and 6
        for (uint32_t p : members[a]) {
            const Box& r = rect_of[p];
            const int w = box[4 * p + 2], h = box[4 * p + 3];
            for (int y = r.min_y; y < r.max_y; ++y) for (int x = r.min_x; x < r.max_x; ++x) owner[(size_t)y * size + x] = (int32_t)p;
            for (int i = 0; i < w + 2 * padding; ++i) {
                for (int j = 0; j < h + 2 * padding; ++j) {
                    const int sx = i - padding, sy = j - padding;
                    if (sx < 0 || sx >= w || sy < 0 || sy >= h) continue;
                    const size_t src = (size_t)pix_ptr[p] + (size_t)sy * w + sx, dst = (size_t)(r.min_y + j) * size + (r.min_x + i);
                    for (int c = 0; c < 3; ++c) img[3 * dst + c] = float_to_byte(pimage[3 * src + c]);
                    mask[dst] = pvalid[src];
                    if (pvalid[src] == 255) source[dst] = (int32_t)p;
                }
            }
            const float ox = (float)(r.min_x + padding), oy = (float)(r.min_y + padding);
            for (uint32_t e = fptr[p]; e < fptr[p + 1]; ++e) {
                M.faces.push_back(pfaces[e]);
                for (int k = 0; k < 3; ++k) {
                    float tx = ptc[6 * (size_t)e + 2 * k] + ox, ty = ptc[6 * (size_t)e + 2 * k + 1] + oy;
                    tx = tx / size; ty = ty / size;
                    if (!std::isfinite(tx) || !std::isfinite(ty)) { M.status = ST_UNSUPPORTED; return; }   // merge_texcoords has no order for a NaN: refused
                    tcs.emplace_back(tx, ty);
                    M.texcoords.push_back(tx); M.texcoords.push_back(ty);
                }
            }
        }
        M.face_ptr[a + 1] = (uint32_t)M.faces.size();
        for (size_t i = 0; i < mask.size(); ++i) if (mask[i] == 255) ++M.stats[S_VALID];
        // item 7
        const float gauss[9] = {1.0f / 16.0f, 2.0f / 16.0f, 1.0f / 16.0f, 2.0f / 16.0f, 4.0f / 16.0f, 2.0f / 16.0f, 1.0f / 16.0f, 2.0f / 16.0f, 1.0f / 16.0f};
        auto in = [&](int x, int y) { return 0 <= x && x < size && 0 <= y && y < size; };
        std::set<std::pair<int, int>> frontier;
        for (int y = 0; y < size; ++y) for (int x = 0; x < size; ++x) {
            if (mask[(size_t)y * size + x] == 255) continue;
            for (int j = -1; j <= 1; ++j) for (int i = -1; i <= 1; ++i)
                if (in(x + i, y + j) && mask[(size_t)(y + j) * size + x + i] == 255) frontier.insert(std::make_pair(x, y));
        }
        std::vector<uint8_t> nmask(mask);
        for (int n = 0; n <= padding; ++n) {
            std::vector<std::pair<int, int>> fresh;
            for (auto it = frontier.begin(); it != frontier.end(); ++it) {
                const int x = it->first, y = it->second;
                bool now_valid = false;
                for (int c = 0; c < 3; ++c) {
                    float norm = 0.0f, value = 0.0f;
                    for (int j = -1; j <= 1; ++j) for (int i = -1; i <= 1; ++i) {
                        const int nx = x + i, ny = y + j;
                        if (in(nx, ny) && nmask[(size_t)ny * size + nx] == 255) {
                            const float w = gauss[(j + 1) * 3 + (i + 1)];
                            norm += w;
                            value += (img[3 * ((size_t)ny * size + nx) + c] / 255.0f) * w;
                            if (c == 0 && source[(size_t)y * size + x] < 0) source[(size_t)y * size + x] = source[(size_t)ny * size + nx];
                        }
                    }
                    if (norm == 0.0f) continue;
                    now_valid = true;
                    img[3 * ((size_t)y * size + x) + c] = (uint8_t)((value / norm) * 255.0f);
                }
                if (now_valid) fresh.push_back(*it);
            }
            frontier.clear();
            for (auto& q : fresh) {
                const size_t i = (size_t)q.second * size + q.first;
                nmask[i] = 255; ++M.stats[S_PADDED];
                if (owner[i] >= 0 && source[i] >= 0 && owner[i] != source[i]) ++M.counters[C_FOREIGN_FILL];
                if (n == padding) ++M.counters[C_OUTER_RING];
            }
            for (auto& q : fresh)
                for (int j = -1; j <= 1; ++j) for (int i = -1; i <= 1; ++i) {
                    const int nx = q.first + i, ny = q.second + j;
                    if (in(nx, ny) && nmask[(size_t)ny * size + nx] == 0) frontier.insert(std::make_pair(nx, ny));
                }
        }
        // item 8
        std::map<std::pair<float, float>, size_t, VecLess> seen;
        size_t n_merged = 0;
        for (auto& tc : tcs) {
            auto it = seen.find(tc);
            if (it == seen.end()) {
                seen[tc] = n_merged; M.texcoord_ids.push_back((uint32_t)n_merged); ++n_merged;
                M.texcoords_merged.push_back(tc.first); M.texcoords_merged.push_back(tc.second);
            } else {
                M.texcoord_ids.push_back((uint32_t)it->second);
            }
        }
        M.tc_ptr[a + 1] = M.tc_ptr[a] + (uint32_t)n_merged;
        M.stats[S_MERGED] += n_merged;
    }
    M.ms_total = now_ms() - t0;
}

}  // namespace

extern "C" {

void* atlas_model_run(uint32_t NP, const int32_t* box, const uint32_t* face_ptr, const uint32_t* faces, const float* texcoords, const uint64_t* pix_ptr,
                      const float* image, const uint8_t* validity, int pack_only) {
    Model* M = new Model();
    run(*M, NP, box, face_ptr, faces, texcoords, pix_ptr, image, validity, pack_only != 0);
    return M;
}
int atlas_model_status(void* h) { return ((Model*)h)->status; }
void atlas_model_stats(void* h, uint64_t* stats, uint64_t* counters, double* ms) {
    Model* M = (Model*)h;
    memcpy(stats, M->stats, sizeof(M->stats)); memcpy(counters, M->counters, sizeof(M->counters));
    ms[0] = M->ms_pack; ms[1] = M->ms_total;
}
const void* atlas_model_array(void* h, const char* name, uint64_t* n) {
    Model* M = (Model*)h;
    const std::string s(name);
#define ARR(NAME) if (s == #NAME) { *n = M->NAME.size(); return M->NAME.data(); }
    ARR(atlas_size) ARR(atlas_pix_ptr) ARR(image) ARR(patch_atlas) ARR(patch_pos) ARR(patch_order) ARR(face_ptr) ARR(faces) ARR(texcoords) ARR(tc_ptr)
    ARR(texcoords_merged) ARR(texcoord_ids)
#undef ARR
    *n = 0; return nullptr;
}
void atlas_model_free(void* h) { delete (Model*)h; }
// one bin alone (item 3): rectangles (w, h) offered in order to a bin of size x size; out[3 k ..] = placed, min_x, min_y
void atlas_model_bin(uint32_t size, uint32_t n, const int32_t* wh, int32_t* out) {
    Bin bin(size, size);
    for (uint32_t k = 0; k < n; ++k) {
        Box r{0, 0, wh[2 * k], wh[2 * k + 1]};
        const bool ok = bin.insert(&r);
        out[3 * k] = ok ? 1 : 0; out[3 * k + 1] = ok ? r.min_x : 0; out[3 * k + 2] = ok ? r.min_y : 0;
    }
}

}  // extern "C"
