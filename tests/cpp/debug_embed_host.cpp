// The host side of csrc/debug_embed.h behind a C interface, for tests/test_debug_embeddings.py (g++, no HIP).
#include "debug_embed.h"

extern "C" {
void dbg_table(uint32_t* style, float* lum, float* prod) { mvs::debug_style_table(style, lum, prod); }
void dbg_image(int w, int h, uint32_t id, uint32_t position, uint8_t* rgb) { mvs::debug_image_host(w, h, id, position, rgb); }
int dbg_pixel(int x, int y, int w, int h, uint32_t id) { return mvs::debug_pixel(x, y, w, h, id) ? 1 : 0; }
}
