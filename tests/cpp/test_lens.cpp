// test_lens.cpp -- csrc/lens.h on the host, stand-alone (its own main; built with the address and undefined-behaviour sanitizers by
// tests/test_lens_host.py).  argv[1]: a directory with `manifest`, one line per image: <name> <width> <height> <flen> <dist0> <dist1>.
// <name>.rgb ([height][width][3]) is undistorted by the twin into <name>.out, which the test compares with the oracle.  Both buffers hold
// exactly the image's bytes on the heap, so that a read or write past an end is a sanitizer report.  The lens checks are run too.
#include <stdio.h>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <vector>

#include "lens.h"

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
        std::string name; int w = 0, h = 0; double flen = 0, d0 = 0, d1 = 0;
        ls >> name >> w >> h >> flen >> d0 >> d1;
        if (!ls || w < 1 || h < 1) { printf("FAIL bad manifest line: %s\n", line.c_str()); ++failures; continue; }
        std::vector<uint8_t> in = slurp(dir + "/" + name + ".rgb");
        in.shrink_to_fit();
        if (in.size() != (size_t)w * h * 3) { printf("FAIL %s: %zu bytes for %d x %d\n", name.c_str(), in.size(), w, h); ++failures; continue; }
        std::vector<uint8_t> out(in.size(), 0xAB);
        out.shrink_to_fit();
        const uint64_t none = mvs::undistort_image_host(in.data(), w, h, (float)flen, (float)d0, (float)d1, out.data());
        uint64_t black = 0;
        for (size_t p = 0; p < in.size(); p += 3) black += (out[p] | out[p + 1] | out[p + 2]) == 0 ? 1 : 0;
        if (none != black) { printf("FAIL %s: %llu pixels without a source, %llu black ones\n", name.c_str(), (unsigned long long)none, (unsigned long long)black); ++failures; }   // (the inputs have no black pixel)
        std::ofstream o(dir + "/" + name + ".out", std::ios::binary);
        o.write((const char*)out.data(), (std::streamsize)out.size());
        ++images;
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const struct { mvs_lens L; bool good; } checks[] = {{{1.0f, 0.1f, 0.0f, 0u}, true}, {{0.0f, 0.0f, 0.5f, 0u}, true}, {{0.0f, 0.1f, 0.0f, 0u}, false}, {{-1.0f, 0.1f, 0.0f, 0u}, false},
                                                       {{1.0f, 0.1f, nan, 0u}, false}, {{nan, 0.0f, 0.0f, 0u}, false}, {{1.0f, inf, 0.0f, 0u}, false}, {{1.0f, 0.1f, 0.0f, 1u}, false}};
    for (const auto& c : checks)
        if (mvs::lens_refusal(c.L).empty() != c.good) { printf("FAIL lens_refusal(%g, %g, %g, %u)\n", c.L.flen, c.L.dist0, c.L.dist1, c.L.reserved); ++failures; }
    printf("images %d\nfailures %d\n", images, failures);
    return failures ? 1 : 0;
}
