// Undoes the PNG row filters 0 .. 4 of an 8-bit RGB image (3 bytes per pixel) for tests/tools/png_decode.py, which builds this file on
// first use: Average and Paeth depend on the decoded byte to the left, which numpy cannot express without a loop over the row.
// raw: h rows of one filter byte + 3 w filtered bytes; out: h * 3 w bytes.  Returns 0, or 1 + the row of the first filter byte above 4.
// Written from the PNG specification, independently of csrc/png_rle.h.  Test infrastructure only.
#include <stdint.h>
#include <stdlib.h>

extern "C" int png_unfilter_rgb8(const uint8_t* raw, uint32_t w, uint32_t h, uint8_t* out) {
    const size_t rb = 3 * (size_t)w;
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t* in = raw + (size_t)y * (rb + 1);
        uint8_t* cur = out + (size_t)y * rb;
        const uint8_t* up = y ? cur - rb : nullptr;
        const int t = in[0];
        if (t > 4) return 1 + (int)y;
        for (size_t x = 0; x < rb; ++x) {
            const int a = x >= 3 ? cur[x - 3] : 0, b = up ? up[x] : 0, c = (up && x >= 3) ? up[x - 3] : 0;
            int pred = 0;
            switch (t) {
                case 1: pred = a; break;
                case 2: pred = b; break;
                case 3: pred = (a + b) / 2; break;
                case 4: {
                    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    break;
                }
                default: break;
            }
            cur[x] = (uint8_t)(in[1 + x] + pred);
        }
    }
    return 0;
}
