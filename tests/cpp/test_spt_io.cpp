// The .spt reader and writer and the .vec writer (csrc/spt_io.h) on their own, on tiny temporary files: the round trip, and every way
// a file can lie to the reader (each refusal is pinned to its own message: a reader that allocated what a lying header announces and
// then ran out of file would say something else).  Built with -fsanitize=address,undefined by tests/test_spt_io_host.py; argv[1] = a
// directory to write in.  Prints "ok" and exits 0, or says which check failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "spt_io.h"

using namespace mvs;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static std::string g_dir;
static std::string path_of(const char* name) { return g_dir + "/" + name; }
static std::string bytes_of(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb"); CHECK(f != nullptr);
    std::string s; char buf[4096]; size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}
static std::string put(const char* name, const std::string& bytes) {
    const std::string p = path_of(name);
    FILE* f = fopen(p.c_str(), "wb"); CHECK(f != nullptr);
    CHECK(fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size());
    CHECK(fclose(f) == 0);
    return p;
}
static std::string record(uint32_t col, uint16_t row, float v) {
    char r[10]; memcpy(r, &col, 4); memcpy(r + 4, &row, 2); memcpy(r + 6, &v, 4);
    return std::string(r, 10);
}
static void release(mvs_csr* c) { free(c->col_ptr); free(c->view_id); free(c->cost); memset(c, 0, sizeof(*c)); }
static bool all_zero(const mvs_csr& c) { return c.n_faces == 0 && c.n_views == 0 && c.nnz == 0 && !c.col_ptr && !c.view_id && !c.cost; }
// the reader refuses `bytes` with exactly this message and hands back nothing
static void refused(const char* name, const std::string& bytes, const char* message) {
    const std::string p = put(name, bytes);
    mvs_csr out; memset(&out, 0xFF, sizeof(out));   // (whatever the caller had there)
    std::string msg;
    CHECK(read_spt(p.c_str(), &out, msg) == MVS_ERR_INVALID);
    if (msg != message) { fprintf(stderr, "%s: message \"%s\", expected \"%s\"\n", name, msg.c_str(), message); exit(1); }
    CHECK(all_zero(out));
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    g_dir = argv[1];
    std::string msg;

    // ---- round trip: 6 columns, the first, a middle and the last one empty; read -> write reproduces the bytes ----
    {
        uint32_t col_ptr[7] = {0, 0, 2, 3, 3, 6, 6};
        uint16_t view_id[6] = {1, 4, 0, 2, 3, 65534};
        float cost[6] = {0.25f, 1.0f, 0.0f, 0.5f, 0.125f, 0.75f};
        mvs_csr t; t.n_faces = 6; t.n_views = 65535; t.nnz = 6; t.col_ptr = col_ptr; t.view_id = view_id; t.cost = cost;
        const std::string p = path_of("round.spt"), p2 = path_of("round2.spt");
        CHECK(write_spt(&t, p.c_str(), msg) == MVS_OK);
        std::string expect = "SPT 0.2 6 65535 6\n";
        for (uint32_t c = 0; c < 6; ++c) for (uint32_t k = col_ptr[c]; k < col_ptr[c + 1]; ++k) expect += record(c, view_id[k], cost[k]);
        CHECK(bytes_of(p) == expect);
        mvs_csr got;
        CHECK(read_spt(p.c_str(), &got, msg) == MVS_OK);
        CHECK(got.n_faces == 6 && got.n_views == 65535 && got.nnz == 6);
        CHECK(memcmp(got.col_ptr, col_ptr, sizeof(col_ptr)) == 0 && memcmp(got.view_id, view_id, sizeof(view_id)) == 0 && memcmp(got.cost, cost, sizeof(cost)) == 0);
        CHECK(write_spt(&got, p2.c_str(), msg) == MVS_OK);
        CHECK(bytes_of(p2) == expect);
        release(&got);

        // trailing bytes after the last record are accepted
        const std::string p3 = put("trailing.spt", expect + "xyz");
        CHECK(read_spt(p3.c_str(), &got, msg) == MVS_OK);
        CHECK(got.nnz == 6 && memcmp(got.col_ptr, col_ptr, sizeof(col_ptr)) == 0 && memcmp(got.view_id, view_id, sizeof(view_id)) == 0);
        release(&got);
    }
    // ---- more than one 1 MB write block: 110000 records in one column ----
    {
        const uint32_t n = 110000;
        std::vector<uint16_t> view(n); std::vector<float> cost(n);
        for (uint32_t k = 0; k < n; ++k) { view[k] = (uint16_t)(k % 60000); cost[k] = (float)k; }
        uint32_t col_ptr[3] = {0, n, n};
        mvs_csr t; t.n_faces = 2; t.n_views = 60000; t.nnz = n; t.col_ptr = col_ptr; t.view_id = view.data(); t.cost = cost.data();
        const std::string p = path_of("blocks.spt");
        CHECK(write_spt(&t, p.c_str(), msg) == MVS_OK);
        CHECK(bytes_of(p).size() == strlen("SPT 0.2 2 60000 110000\n") + 10u * n);
        mvs_csr got;
        CHECK(read_spt(p.c_str(), &got, msg) == MVS_OK);
        CHECK(got.nnz == n && got.col_ptr[0] == 0 && got.col_ptr[1] == n && got.col_ptr[2] == n);
        CHECK(memcmp(got.view_id, view.data(), n * sizeof(uint16_t)) == 0 && memcmp(got.cost, cost.data(), n * sizeof(float)) == 0);
        release(&got);
    }
    // ---- the empty table ----
    {
        const std::string p = put("empty.spt", "SPT 0.2 0 0 0\n");
        mvs_csr got;
        CHECK(read_spt(p.c_str(), &got, msg) == MVS_OK);
        CHECK(got.n_faces == 0 && got.n_views == 0 && got.nnz == 0 && got.col_ptr && got.col_ptr[0] == 0);
        const std::string p2 = path_of("empty2.spt");
        CHECK(write_spt(&got, p2.c_str(), msg) == MVS_OK);
        CHECK(bytes_of(p2) == "SPT 0.2 0 0 0\n");
        release(&got);
    }
    // ---- lying files ----
    const std::string three = record(0, 0, 1.0f) + record(1, 1, 2.0f) + record(2, 2, 3.0f);   // a 30-byte body
    refused("magic.spt", "SPX 0.2 3 3 3\n" + three, "Not a SparseTable file!");
    refused("short_header.spt", "SPT 0.2 3\n", "Not a SparseTable file!");
    refused("nothing.spt", "", "Not a SparseTable file!");
    refused("version.spt", "SPT 0.3 3 3 3\n" + three, "Incompatible version of SparseTable file!");
    // more records announced than the rest of the file holds: refused before anything is allocated (0xFFFFFFEF records would be 25 GB)
    refused("nnz_one_more.spt", "SPT 0.2 3 3 4\n" + three, "corrupt SparseTable file (record count exceeds the file)");
    refused("nnz_huge.spt", "SPT 0.2 3 3 4294967279\n" + three, "corrupt SparseTable file (record count exceeds the file)");
    refused("nnz_limit.spt", "SPT 0.2 3 3 4294967280\n" + three, "corrupt SparseTable file (record count exceeds the file)");
    refused("nnz_64bit.spt", "SPT 0.2 3 3 18446744073709551615\n" + three, "corrupt SparseTable file (record count exceeds the file)");
    refused("truncated.spt", "SPT 0.2 3 3 3\n" + three.substr(0, 29), "corrupt SparseTable file (record count exceeds the file)");
    // bad records: out is zeroed although the arrays were allocated by then
    refused("col_range.spt", "SPT 0.2 3 3 3\n" + record(0, 0, 1.0f) + record(3, 1, 2.0f) + record(2, 2, 3.0f), "corrupt SparseTable file");
    refused("col_descending.spt", "SPT 0.2 3 3 3\n" + record(0, 0, 1.0f) + record(2, 1, 2.0f) + record(1, 2, 3.0f), "corrupt SparseTable file");
    refused("row_range.spt", "SPT 0.2 3 3 3\n" + record(0, 0, 1.0f) + record(1, 3, 2.0f) + record(2, 2, 3.0f), "corrupt SparseTable file");
    {   // (the same three records, well-formed, are read)
        const std::string p = put("three.spt", "SPT 0.2 3 3 3\n" + three);
        mvs_csr got;
        CHECK(read_spt(p.c_str(), &got, msg) == MVS_OK);
        CHECK(got.col_ptr[3] == 3 && got.view_id[2] == 2 && got.cost[1] == 2.0f);
        release(&got);
    }
    // ---- files that cannot be opened, null arguments ----
    {
        const std::string missing = path_of("no_such_directory/x.spt");
        mvs_csr out; memset(&out, 0xFF, sizeof(out));
        CHECK(read_spt(missing.c_str(), &out, msg) == MVS_ERR_INVALID && msg == "cannot open " + missing && all_zero(out));
        uint32_t col_ptr[1] = {0};
        mvs_csr t; memset(&t, 0, sizeof(t)); t.col_ptr = col_ptr;
        msg.clear();
        CHECK(write_spt(&t, missing.c_str(), msg) == MVS_ERR_INVALID && msg == "cannot open " + missing);
        const uint32_t labels[1] = {0};
        msg.clear();
        CHECK(write_labeling_vec(labels, 1, missing.c_str(), msg) == MVS_ERR_INVALID && msg == "cannot open " + missing);
        CHECK(read_spt(nullptr, &out, msg) == MVS_ERR_INVALID && msg == "null argument");
        CHECK(read_spt(missing.c_str(), nullptr, msg) == MVS_ERR_INVALID && write_spt(nullptr, missing.c_str(), msg) == MVS_ERR_INVALID);
        CHECK(write_labeling_vec(nullptr, 0, missing.c_str(), msg) == MVS_ERR_INVALID && msg == "null argument");
    }
    // ---- .vec: 8 bytes per label, little endian as the host writes a size_t ----
    {
        const uint32_t labels[4] = {0, 1, 65535, 0xFFFFFFFFu};
        const std::string p = path_of("labels.vec");
        CHECK(write_labeling_vec(labels, 4, p.c_str(), msg) == MVS_OK);
        const std::string b = bytes_of(p);
        CHECK(b.size() == 32);
        for (int i = 0; i < 4; ++i) { uint64_t v; memcpy(&v, b.data() + 8 * i, 8); CHECK(v == labels[i]); }
        CHECK(write_labeling_vec(labels, 0, p.c_str(), msg) == MVS_OK && bytes_of(p).empty());
    }
    printf("ok\n");
    return 0;
}
