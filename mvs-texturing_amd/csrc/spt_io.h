// spt_io.h -- the two file formats of the file-level boundary: SparseTable's .spt and the labeling's .vec (plain host C++, no HIP;
// tests/cpp/test_spt_io.cpp feeds the reader malformed files).  Every function returns the call's status and, when that is not MVS_OK,
// leaves the message in `msg`.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mvs_viewsel.h"

namespace mvs {

namespace spt_detail {
struct FileCloser { void operator()(FILE* f) const { if (f) fclose(f); } };
using File = std::unique_ptr<FILE, FileCloser>;
inline mvs_status fail(std::string& msg, const std::string& what) { msg = what; return MVS_ERR_INVALID; }
}  // namespace spt_detail

/* SparseTable::save_to_file (sparse_table.h:112-136): "SPT 0.2 <cols> <rows> <nnz>\n" then
 * nnz records {u32 col; u16 row; f32 value}, column by column */
inline mvs_status write_spt(const mvs_csr* csr, const char* path, std::string& msg) {
    if (!csr || !path) return spt_detail::fail(msg, "null argument");
    spt_detail::File file(fopen(path, "wb"));
    FILE* f = file.get();
    if (!f) return spt_detail::fail(msg, std::string("cannot open ") + path);
    bool ok = fprintf(f, "SPT 0.2 %u %u %llu\n", csr->n_faces, csr->n_views, (unsigned long long)csr->nnz) > 0;
    // 10-byte records assembled in a 1 MB block and written in one call each (config 3 has 89 M of them)
    std::vector<unsigned char> block; block.reserve((1u << 20) + 16);
    for (uint32_t col = 0; ok && col < csr->n_faces; ++col)
        for (uint32_t k = csr->col_ptr[col]; ok && k < csr->col_ptr[col + 1]; ++k) {
            unsigned char rec[10];
            memcpy(rec, &col, 4); memcpy(rec + 4, &csr->view_id[k], 2); memcpy(rec + 6, &csr->cost[k], 4);
            block.insert(block.end(), rec, rec + 10);
            if (block.size() >= (1u << 20)) { ok = fwrite(block.data(), 1, block.size(), f) == block.size(); block.clear(); }
        }
    if (ok && !block.empty()) ok = fwrite(block.data(), 1, block.size(), f) == block.size();
    if (fclose(file.release()) != 0) ok = false;   // a full disk shows up here at the latest
    return ok ? MVS_OK : spt_detail::fail(msg, std::string("write error on ") + path);
}

/* SparseTable::load_from_file (sparse_table.h:138-187).  *out: the whole table (arrays from malloc: mvs_csr_free), or all zero */
inline mvs_status read_spt(const char* path, mvs_csr* out, std::string& msg) {
    if (!path || !out) return spt_detail::fail(msg, "null argument");
    memset(out, 0, sizeof(*out));
    spt_detail::File file(fopen(path, "rb"));
    FILE* f = file.get();
    if (!f) return spt_detail::fail(msg, std::string("cannot open ") + path);
    char header[16] = {0}, version[16] = {0};
    unsigned cols = 0, rows = 0; unsigned long long nnz = 0;
    if (fscanf(f, "%15s %15s %u %u %llu", header, version, &cols, &rows, &nnz) != 5 || strcmp(header, "SPT") != 0) return spt_detail::fail(msg, "Not a SparseTable file!");
    if (strcmp(version, "0.2") != 0) return spt_detail::fail(msg, "Incompatible version of SparseTable file!");
    int ch; while ((ch = fgetc(f)) != EOF && ch != '\n') {}
    // the header is untrusted: the records it announces must fit in what is left of the file before anything is allocated
    const long data_begin = ftell(f);
    if (data_begin < 0 || fseek(f, 0, SEEK_END) != 0) return spt_detail::fail(msg, "corrupt SparseTable file");
    const long file_end = ftell(f);
    if (file_end < data_begin || nnz > (unsigned long long)(file_end - data_begin) / 10ull || nnz >= 0xFFFFFFF0ull || fseek(f, data_begin, SEEK_SET) != 0)
        return spt_detail::fail(msg, "corrupt SparseTable file (record count exceeds the file)");
    struct Guard {   // all of the caller's arrays or none: on failure what mvs_csr_free does (api.hip; this header stands alone)
        mvs_csr* o; bool keep = false;
        ~Guard() { if (keep) return; free(o->col_ptr); free(o->view_id); free(o->cost); memset(o, 0, sizeof(*o)); }
    } guard{out};
    out->n_faces = cols; out->n_views = rows; out->nnz = nnz;
    out->col_ptr = (uint32_t*)calloc((size_t)cols + 1, sizeof(uint32_t));
    out->view_id = (uint16_t*)malloc((nnz + 1) * sizeof(uint16_t));
    out->cost = (float*)malloc((nnz + 1) * sizeof(float));
    if (!out->col_ptr || !out->view_id || !out->cost) return spt_detail::fail(msg, "out of memory reading the SparseTable file");
    uint32_t prev = 0;
    for (unsigned long long i = 0; i < nnz; ++i) {
        uint32_t col; uint16_t row; float v;
        if (fread(&col, 4, 1, f) != 1 || fread(&row, 2, 1, f) != 1 || fread(&v, 4, 1, f) != 1 || col >= cols || col < prev || row >= rows) return spt_detail::fail(msg, "corrupt SparseTable file");
        prev = col;
        out->col_ptr[col + 1]++; out->view_id[i] = row; out->cost[i] = v;
    }
    for (uint32_t c = 0; c < cols; ++c) out->col_ptr[c + 1] += out->col_ptr[c];
    guard.keep = true;
    return MVS_OK;
}

/* vector_to_file<std::size_t> (util.h:104-113) as used at texrecon.cpp:130-136 */
inline mvs_status write_labeling_vec(const uint32_t* labels, uint32_t n_faces, const char* path, std::string& msg) {
    if (!labels || !path) return spt_detail::fail(msg, "null argument");
    spt_detail::File file(fopen(path, "wb"));
    FILE* f = file.get();
    if (!f) return spt_detail::fail(msg, std::string("cannot open ") + path);
    bool ok = true;
    for (uint32_t i = 0; ok && i < n_faces; ++i) { const uint64_t v = labels[i]; ok = fwrite(&v, sizeof(uint64_t), 1, f) == 1; }
    if (fclose(file.release()) != 0) ok = false;
    return ok ? MVS_OK : spt_detail::fail(msg, std::string("write error on ") + path);
}

}  // namespace mvs
