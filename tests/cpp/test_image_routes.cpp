// Stand-alone host program for the parts of csrc/rows.h and csrc/image_routes.h that make no HIP call: for_each_on_threads, the hand-over
// of finished files (EncodedFiles, files_to_set), the host twins' hand-over (twin_out) and the rules of an image set (check_image_set).
// tests/test_image_routes_host.py compiles it host-only with -fsanitize=address,undefined; prints "ok" and exits 0, or says which check failed.
#include "image_routes.h"

#include <mutex>
#include <set>

namespace mvs {
static std::string g_last;
mvs_status api_fail(mvs_status st, const std::string& msg) { g_last = msg; return st; }   // (api.hip's, which is not linked here)
}  // namespace mvs
using namespace mvs;

#define CHECK(c) do { if (!(c)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static std::string refusal(const ImageSet& S) {
    try { check_image_set(S, "who"); } catch (const StatusError& e) { return e.st == MVS_ERR_INVALID ? e.what() : "wrong status"; }
    return "";
}

int main() {
    // ---- for_each_on_threads: every item once, on min(16, n) threads at the most ----
    for (uint32_t n : {0u, 1u, 5u, 16u, 17u, 1000u}) {
        std::vector<int> hits(n, 0);
        std::mutex m; std::set<std::thread::id> ids;
        for_each_on_threads(n, [&](uint32_t i) { hits[i] += 1; std::lock_guard<std::mutex> g(m); ids.insert(std::this_thread::get_id()); });
        for (int h : hits) CHECK(h == 1);
        CHECK(ids.size() <= std::min<size_t>(16, n));
        CHECK(n == 0 || ids.count(std::this_thread::get_id()) || n > 1);   // (a lone item runs on the calling thread)
        if (n == 1) CHECK(ids.count(std::this_thread::get_id()) == 1);
    }
    // ---- EncodedFiles -> mvs_png_set: the bytes move, the offsets are copied ----
    {
        EncodedFiles F;
        F.offsets = {0, 3, 3, 10};
        F.resize_data();
        for (int i = 0; i < 10; ++i) F.data[i] = (uint8_t)(i + 1);
        const uint8_t* bytes = F.data;
        mvs_png_set out{};
        files_to_set(F, 3, &out);
        CHECK(out.n_images == 3 && out.n_bytes == 10 && out.data == bytes && F.data == nullptr);
        CHECK(out.offsets != F.offsets.data() && memcmp(out.offsets, F.offsets.data(), 4 * sizeof(uint64_t)) == 0 && out.data[9] == 10);
        free(out.data); free(out.offsets);
        EncodedFiles E;                      // no image: one offset, one byte of room
        E.offsets = {0};
        E.resize_data(); E.resize_data();
        CHECK(E.data != nullptr);
        mvs_png_set none{};
        files_to_set(E, 0, &none);
        CHECK(none.n_images == 0 && none.n_bytes == 0 && none.offsets[0] == 0);
        free(none.data); free(none.offsets);
    }
    // ---- twin_out ----
    {
        uint8_t* p = nullptr; uint64_t n = 77;
        const std::vector<uint8_t> v = {9, 8, 7};
        CHECK(twin_out(MVS_OK, "", v, &p, &n) == MVS_OK && n == 3 && p && p != v.data() && memcmp(p, v.data(), 3) == 0);
        free(p); p = nullptr;
        CHECK(twin_out(MVS_OK, "", {}, &p, &n) == MVS_OK && n == 0 && p);
        free(p); p = nullptr; n = 77;
        CHECK(twin_out(MVS_ERR_UNSUPPORTED, "too wide", v, &p, &n) == MVS_ERR_UNSUPPORTED && !p && n == 77 && g_last == "too wide");
    }
    // ---- check_image_set ----
    CHECK(refusal(ImageSet{{}, {}, {0}}) == "");
    CHECK(refusal(ImageSet{{2, 1}, {3, 5}, {0, 6, 11}}) == "");
    CHECK(refusal(ImageSet{{}, {}, {1}}) == "who: pix_ptr does not start at 0");
    CHECK(refusal(ImageSet{{2}, {3}, {1, 7}}) == "who: pix_ptr does not start at 0");
    CHECK(refusal(ImageSet{{0}, {3}, {0, 0}}) == "who: image 0: width, height and pix_ptr do not agree");
    CHECK(refusal(ImageSet{{2, 1}, {3, 0}, {0, 6, 6}}) == "who: image 1: width, height and pix_ptr do not agree");
    CHECK(refusal(ImageSet{{2, 1}, {3, 5}, {0, 6, 10}}) == "who: image 1: width, height and pix_ptr do not agree");
    CHECK(refusal(ImageSet{{2, 1}, {3, 5}, {0, 6, 5}}) == "who: image 1: width, height and pix_ptr do not agree");
    CHECK(refusal(ImageSet{{65536}, {65536}, {0, 0}}) == "who: image 0: width, height and pix_ptr do not agree");   // 2^32 pixels: no 32-bit product
    CHECK(refusal(ImageSet{{65536}, {65536}, {0, 1ull << 32}}) == "");
    puts("ok");
    return 0;
}
