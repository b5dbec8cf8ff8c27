// test_level.cpp -- csrc/level.h on the host, stand-alone (its own main; built with the address and undefined-behaviour sanitizers by
// tests/test_view_levels_host.py).  argv[1]: a directory with `manifest`, one line per image: <name> <width> <height> <level>.
// <name>.rgb ([height][width][3]) is halved `level` times by the twin into <name>.out, which the test compares with its numpy model.
// Both buffers hold exactly the image's bytes on the heap, so that a read or write past an end is a sanitizer report.  The keep rule in
// the bit domain (keep_half_pair) is checked against the AND of neighbouring bits written out.
#include <stdio.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

#include "level.h"

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::ifstream man(dir + "/manifest");
    std::string line;
    int failures = 0, images = 0;
    while (std::getline(man, line)) {
        std::istringstream ls(line);
        std::string name; int w = 0, h = 0; unsigned level = 0;
        ls >> name >> w >> h >> level;
        if (!ls || w < 1 || h < 1 || level > mvs::LEVEL_MAX) { printf("FAIL bad manifest line: %s\n", line.c_str()); ++failures; continue; }
        std::vector<uint8_t> in = slurp(dir + "/" + name + ".rgb");
        in.shrink_to_fit();
        if (in.size() != (size_t)w * h * 3) { printf("FAIL %s: %zu bytes for %d x %d\n", name.c_str(), in.size(), w, h); ++failures; continue; }
        std::vector<uint8_t> out((size_t)mvs::level_dim(w, level) * mvs::level_dim(h, level) * 3, 0xAB);
        out.shrink_to_fit();
        mvs::halve_image_host(in.data(), w, h, 3, level, out.data());
        std::ofstream o(dir + "/" + name + ".out", std::ios::binary);
        o.write((const char*)out.data(), (std::streamsize)out.size());
        ++images;
    }
    // keep_half_pair: bit b of the result is (bit 2b AND bit 2b + 1) of the 64 bits hi:lo
    uint32_t x = 0x9E3779B9u;
    for (int it = 0; it < 2000; ++it) {
        x = x * 1664525u + 1013904223u; const uint32_t lo = it % 7 == 0 ? 0xFFFFFFFFu : x;
        x = x * 1664525u + 1013904223u; const uint32_t hi = it % 5 == 0 ? 0xFFFFFFFFu : x | (x >> 3);
        uint32_t want = 0;
        for (int b = 0; b < 32; ++b) {
            const uint32_t src = b < 16 ? lo : hi; const int p = 2 * (b & 15);
            if (((src >> p) & 1u) && ((src >> (p + 1)) & 1u)) want |= 1u << b;
        }
        if (mvs::keep_half_pair(lo, hi) != want) { printf("FAIL keep_half_pair(%08x, %08x)\n", lo, hi); ++failures; }
    }
    printf("images %d\nfailures %d\n", images, failures);
    return failures ? 1 : 0;
}
