// test_png_dec.cpp -- csrc/png_dec.h on the host, stand-alone (its own main; built with the address and undefined-behaviour sanitizers
// by tests/test_png_decode_host.py).  argv[1]: a directory with `manifest`, one line per file:
//   good <name>              <name>.png must decode; its pixels go to <name>.rgb ([height][width][3]) and "size <name> <w> <h>" to stdout
//   bad <name> <reason ...>  <name>.png must be refused with MVS_ERR_INVALID and a message that contains the reason
// The chunk walk alone (parse_container, what the device route runs on the host) is called on every file too, and the twin on every
// prefix of the first good file, which ends with an IEND chunk of 12 bytes: the prefix that ends behind the last IDAT is the same image
// (IEND is not required), every other one must be refused, never read past its end.
#include <stdio.h>
#include <fstream>
#include <iostream>
#include <sstream>

#include "png_dec.h"

using namespace mvs::png_dec;

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
        const std::vector<uint8_t> file = slurp(dir + "/" + name + ".png");
        // exactly the file's bytes on the heap, so that a read past the end is a sanitizer report
        std::vector<uint8_t> exact(file.begin(), file.end());
        exact.shrink_to_fit();
        std::vector<uint8_t> rgb, raw; std::string msg; uint32_t w = 0, h = 0; Counts counts;
        const mvs_status st = decode_png(exact.data(), exact.size(), rgb, w, h, &raw, msg, &counts);
        File F; std::string pmsg;
        const mvs_status ps = parse_container(exact.data(), exact.size(), F, pmsg);
        if (kind == "good") {
            if (st != MVS_OK || ps != MVS_OK) { printf("FAIL %s: refused: %s\n", name.c_str(), msg.c_str()); ++failures; continue; }
            if (rgb.size() != (size_t)w * h * 3 || raw.size() != F.raw_bytes || counts.rows[0] + counts.rows[1] + counts.rows[2] + counts.rows[3] + counts.rows[4] != h) {
                printf("FAIL %s: sizes\n", name.c_str()); ++failures; continue;
            }
            std::ofstream o(dir + "/" + name + ".rgb", std::ios::binary);
            o.write((const char*)rgb.data(), (std::streamsize)rgb.size());
            printf("size %s %u %u\n", name.c_str(), w, h);
            if (!cut_done) {
                cut_done = true;
                for (size_t n = 0; n < exact.size(); ++n) {
                    std::vector<uint8_t> cut(exact.begin(), exact.begin() + (std::ptrdiff_t)n);
                    cut.shrink_to_fit();
                    std::vector<uint8_t> r2; std::string m2; uint32_t w2, h2;
                    const mvs_status s2 = decode_png(cut.data(), cut.size(), r2, w2, h2, nullptr, m2);
                    if (n + 12 == exact.size() ? (s2 != MVS_OK || r2 != rgb) : (s2 != MVS_ERR_INVALID || !r2.empty())) {
                        printf("FAIL %s: prefix of %zu bytes: status %d\n", name.c_str(), n, (int)s2); ++failures; break;
                    }
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
