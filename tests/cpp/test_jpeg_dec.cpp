// test_jpeg_dec.cpp -- csrc/jpeg_dec.h on the host, stand-alone (its own main; built with the address and undefined-behaviour sanitizers
// by tests/test_jpeg_decode_host.py).  argv[1]: a directory with `manifest`, one line per file:
//   good <name>              <name>.jpg must decode; its pixels go to <name>.rgb ([height][width][3]) and "size <name> <w> <h> <blocks>" to stdout
//   bad <name> <reason ...>  <name>.jpg must be refused with MVS_ERR_INVALID and a message that contains the reason
// The parser alone (parse_headers, what the device route runs on the host) is called on every file too, and on every prefix of the
// first good file: a cut file must be refused, never read past its end.
#include <stdio.h>
#include <fstream>
#include <iostream>
#include <sstream>

#include "jpeg_dec.h"

using namespace mvs::jpeg_dec;

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::ifstream man(dir + "/manifest");
    std::string line;
    int failures = 0; bool cut_done = false;
    while (std::getline(man, line)) {
        std::istringstream ls(line);
        std::string kind, name, reason;
        ls >> kind >> name;
        std::getline(ls, reason);
        if (!reason.empty() && reason[0] == ' ') reason.erase(0, 1);
        const std::vector<uint8_t> file = slurp(dir + "/" + name + ".jpg");
        // exactly the file's bytes on the heap, so that a read past the end is a sanitizer report
        std::vector<uint8_t> exact(file.begin(), file.end());
        exact.shrink_to_fit();
        std::vector<uint8_t> rgb; std::vector<int16_t> coef; std::string msg; uint32_t w = 0, h = 0;
        const mvs_status st = decode_jpeg(exact.data(), exact.size(), rgb, w, h, &coef, msg);
        Frame F; size_t begin = 0; std::string pmsg;
        const mvs_status ps = parse_headers(exact.data(), exact.size(), F, begin, pmsg);
        if (kind == "good") {
            if (st != MVS_OK || ps != MVS_OK) { printf("FAIL %s: refused: %s\n", name.c_str(), msg.c_str()); ++failures; continue; }
            if (rgb.size() != (size_t)w * h * 3 || coef.size() != (size_t)F.mw * F.mh * F.bpm * 64) { printf("FAIL %s: sizes\n", name.c_str()); ++failures; continue; }
            std::ofstream o(dir + "/" + name + ".rgb", std::ios::binary);
            o.write((const char*)rgb.data(), (std::streamsize)rgb.size());
            printf("size %s %u %u %zu\n", name.c_str(), w, h, coef.size() / 64);
            if (!cut_done) {   // every prefix of a good file is refused
                cut_done = true;
                for (size_t n = 0; n < exact.size(); ++n) {
                    std::vector<uint8_t> cut(exact.begin(), exact.begin() + (std::ptrdiff_t)n);
                    cut.shrink_to_fit();
                    std::vector<uint8_t> r2; std::string m2; uint32_t w2, h2;
                    if (decode_jpeg(cut.data(), cut.size(), r2, w2, h2, nullptr, m2) != MVS_ERR_INVALID) { printf("FAIL %s: prefix of %zu bytes accepted\n", name.c_str(), n); ++failures; break; }
                }
            }
        } else {
            if (st != MVS_ERR_INVALID) { printf("FAIL %s: status %d, expected a refusal\n", name.c_str(), (int)st); ++failures; continue; }
            if (msg.find(reason) == std::string::npos) { printf("FAIL %s: message '%s' lacks '%s'\n", name.c_str(), msg.c_str(), reason.c_str()); ++failures; continue; }
            if (!rgb.empty()) { printf("FAIL %s: pixels beside a refusal\n", name.c_str()); ++failures; continue; }
            printf("refused %s: %s\n", name.c_str(), msg.c_str());
        }
    }
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
