// png_io.h -- the file side of the model output (row f9; DESIGN.md section 4 "Model output" items 4-5): a PNG encoder for 8-bit RGB
// images and the writer of a byte range (plain host C++, no HIP; tests/cpp/test_png_fmt.cpp runs it under the sanitizers).  Every
// function returns the call's status and, when that is not MVS_OK, leaves the message in `msg`.
//   PNG: 8-bit RGB, non-interlaced, filter type 0 on every row, one zlib stream in one IDAT chunk.  level 0: stored deflate blocks of at
//   most 65535 bytes with this file's own CRC-32 and Adler-32 -- no dependency; level 1 .. 9: compress2 of libz.so.1, resolved at run
//   time (MVS_ERR_UNSUPPORTED where it is not found).  Pixel parity with any PNG writer, not byte parity.
#pragma once
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mvs_viewsel.h"

namespace mvs {

namespace png_detail {
struct FileCloser { void operator()(FILE* f) const { if (f) fclose(f); } };
using File = std::unique_ptr<FILE, FileCloser>;
inline mvs_status fail(std::string& msg, mvs_status st, const std::string& what) { msg = what; return st; }

struct Crc32 {   // slicing by eight: t[0] is the byte table, t[k][n] the CRC of byte n followed by k zero bytes
    uint32_t t[8][256];
    Crc32() {
        for (uint32_t n = 0; n < 256; ++n) {
            uint32_t c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][n] = c;
        }
        for (int k = 1; k < 8; ++k)
            for (uint32_t n = 0; n < 256; ++n) t[k][n] = (t[k - 1][n] >> 8) ^ t[0][t[k - 1][n] & 0xFFu];
    }
};
inline uint32_t crc32_update(uint32_t crc, const uint8_t* p, size_t n) {   // crc: the running value, 0xFFFFFFFF at the start, inverted at the end
    static const Crc32 T;
    for (; n >= 8; p += 8, n -= 8) {
        const uint32_t a = crc ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        const uint32_t b = (uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
        crc = T.t[7][a & 0xFFu] ^ T.t[6][(a >> 8) & 0xFFu] ^ T.t[5][(a >> 16) & 0xFFu] ^ T.t[4][a >> 24] ^
              T.t[3][b & 0xFFu] ^ T.t[2][(b >> 8) & 0xFFu] ^ T.t[1][(b >> 16) & 0xFFu] ^ T.t[0][b >> 24];
    }
    for (size_t i = 0; i < n; ++i) crc = T.t[0][(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
    return crc;
}
inline uint32_t adler32_update(uint32_t adler, const uint8_t* p, size_t n) {   // 1 at the start
    uint32_t a = adler & 0xFFFFu, b = adler >> 16;
    while (n) {
        const size_t run = n < 5552 ? n : 5552;   // the longest run whose sums stay below 2^32
        for (size_t i = 0; i < run; ++i) { a += p[i]; b += a; }
        a %= 65521u; b %= 65521u; p += run; n -= run;
    }
    return (b << 16) | a;
}
inline void put_be32(std::vector<uint8_t>& o, uint32_t v) { o.push_back((uint8_t)(v >> 24)); o.push_back((uint8_t)(v >> 16)); o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); }
inline void put_chunk(std::vector<uint8_t>& o, const char type[4], const uint8_t* data, size_t n) {
    put_be32(o, (uint32_t)n);
    const size_t at = o.size();
    o.insert(o.end(), type, type + 4);
    if (n) o.insert(o.end(), data, data + n);
    put_be32(o, ~crc32_update(0xFFFFFFFFu, o.data() + at, n + 4));
}

// compress2 / compressBound of libz.so.1 (null when the library is not there)
struct Zlib {
    int (*compress2)(unsigned char*, unsigned long*, const unsigned char*, unsigned long, int) = nullptr;
    unsigned long (*compressBound)(unsigned long) = nullptr;
};
inline const Zlib& zlib() {
    static const Zlib Z = [] {
        Zlib z;
        void* h = nullptr;
        for (const char* name : {"libz.so.1", "libz.so"}) { h = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (h) break; }
        if (h) {
            z.compress2 = reinterpret_cast<decltype(z.compress2)>(dlsym(h, "compress2"));
            z.compressBound = reinterpret_cast<decltype(z.compressBound)>(dlsym(h, "compressBound"));
            if (!z.compress2 || !z.compressBound) z = Zlib{};
        }
        return z;
    }();
    return Z;
}
}  // namespace png_detail

inline bool png_zlib_available() { return png_detail::zlib().compress2 != nullptr; }

/* the PNG file of rgb [height][width][3] in `out` */
inline mvs_status encode_png(const uint8_t* rgb, uint32_t width, uint32_t height, int level, std::vector<uint8_t>& out, std::string& msg) {
    using namespace png_detail;
    out.clear();
    if (!rgb || !width || !height) return fail(msg, MVS_ERR_INVALID, "write_png: null image or empty frame");
    if (level < 0 || level > 9) return fail(msg, MVS_ERR_INVALID, "write_png: level 0 .. 9");
    const uint64_t row = 3ull * width + 1ull, raw_bytes = row * height;
    if (width > 0x7FFFFFFFu || height > 0x7FFFFFFFu || raw_bytes > 0x7FF00000ull) return fail(msg, MVS_ERR_UNSUPPORTED, "write_png: image too large for one IDAT chunk");
    std::vector<uint8_t> raw((size_t)raw_bytes);   // every row behind its filter byte 0
    for (uint32_t y = 0; y < height; ++y) {
        raw[(size_t)(y * row)] = 0;
        memcpy(&raw[(size_t)(y * row + 1)], rgb + (size_t)y * 3 * width, (size_t)3 * width);
    }
    std::vector<uint8_t> z;
    if (level == 0) {
        const size_t n = raw.size(), blocks = (n + 65534) / 65535;
        z.reserve(n + 5 * blocks + 6);
        z.push_back(0x78); z.push_back(0x01);
        for (size_t at = 0; at < n; at += 65535) {
            const size_t len = n - at < 65535 ? n - at : 65535;
            z.push_back(at + len == n ? 1 : 0);
            z.push_back((uint8_t)len); z.push_back((uint8_t)(len >> 8)); z.push_back((uint8_t)~len); z.push_back((uint8_t)(~len >> 8));
            z.insert(z.end(), raw.begin() + at, raw.begin() + at + len);
        }
        put_be32(z, adler32_update(1u, raw.data(), n));
    } else {
        const Zlib& Z = zlib();
        if (!Z.compress2) return fail(msg, MVS_ERR_UNSUPPORTED, "write_png: libz.so.1 not found (level 0 needs no library)");
        unsigned long zn = Z.compressBound((unsigned long)raw.size());
        if (zn > 0x7FF00000ul) return fail(msg, MVS_ERR_UNSUPPORTED, "write_png: image too large for one IDAT chunk");
        z.resize(zn);
        if (Z.compress2(z.data(), &zn, raw.data(), (unsigned long)raw.size(), level) != 0) return fail(msg, MVS_ERR_INVALID, "write_png: compress2 failed");
        z.resize(zn);
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    out.reserve(z.size() + 64);
    out.insert(out.end(), sig, sig + 8);
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, width); put_be32(ihdr, height);
    const uint8_t tail[5] = {8, 2, 0, 0, 0};   // bit depth, colour type RGB, compression, filter method, no interlace
    ihdr.insert(ihdr.end(), tail, tail + 5);
    put_chunk(out, "IHDR", ihdr.data(), ihdr.size());
    put_chunk(out, "IDAT", z.data(), z.size());
    put_chunk(out, "IEND", nullptr, 0);
    return MVS_OK;
}

inline mvs_status write_file(const char* path, const void* data, size_t n, std::string& msg) {
    if (!path || (n && !data)) return png_detail::fail(msg, MVS_ERR_INVALID, "null argument");
    png_detail::File file(fopen(path, "wb"));
    FILE* f = file.get();
    if (!f) return png_detail::fail(msg, MVS_ERR_INVALID, std::string("cannot open ") + path);
    bool ok = !n || fwrite(data, 1, n, f) == n;
    if (fclose(file.release()) != 0) ok = false;
    return ok ? MVS_OK : png_detail::fail(msg, MVS_ERR_INVALID, std::string("write error on ") + path);
}

inline mvs_status write_png(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height, int level, std::string& msg) {
    if (!path) return png_detail::fail(msg, MVS_ERR_INVALID, "null argument");
    std::vector<uint8_t> png;
    const mvs_status st = encode_png(rgb, width, height, level, png, msg);
    return st != MVS_OK ? st : write_file(path, png.data(), png.size(), msg);
}

}  // namespace mvs
