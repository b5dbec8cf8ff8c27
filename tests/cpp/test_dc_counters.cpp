// The counter slots of the data-cost pass and the statistics made of them (csrc/dc_counters.h) on their own: every slot lands in its
// field, sums over ranges pass 2^32, the two floats come back from their bit patterns.  Built with -fsanitize=address,undefined by
// tests/test_dc_ranges_host.py; prints "ok" and exits 0, or says which check failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dc_counters.h"

using namespace mvs;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static uint32_t bits_of(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static bool same_bits(float a, float b) { return bits_of(a) == bits_of(b); }

int main() {
    // ---- the values the kernels were compiled with ----
    CHECK(C_BACK == 0 && C_ANGLE == 1 && C_OUTSIDE == 2 && C_OCCL == 3 && C_ZEROQ == 4 && C_SURV == 5 && C_RAYS == 6 && C_PASS == 7);
    CHECK(C_RNODES == 8 && C_RTRIS == 9 && C_RPACKETS == 10 && C_RGENERIC == 11 && C_REWALK == 12 && C_RLEAF_ROUNDS == 13);
    CHECK(C_MAX_Q_BITS == 14 && C_PCTL_BITS == 15 && C_PREP == 32 && C_KMAX == 48 && C_N_SLOTS == 64);
    // ---- a block whose every slot holds a distinct prime: field by field ----
    const unsigned long long primes[C_N_STATS] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53};
    {
        mvs_dc_stats S; memset(&S, 0, sizeof(S));
        S.pairs = 1009; S.nnz_pre = 1013;                                       // not the counters' business
        dc_stats_from_counters(primes, 59, 61, &S);
        CHECK(S.cull_backface == 2 && S.cull_angle == 3 && S.cull_outside == 5 && S.cull_occluded == 7 && S.cull_zero_quality == 11);
        CHECK(S.rays == 17 && S.ray_nodes == 23 && S.ray_packets == 31 && S.ray_packets_generic == 37 && S.ray_leaf_rounds == 43);
        CHECK(S.ray_tris == 16 * 29);                                            // leaf visits x 16 triangles
        CHECK(S.footprints_rewalked == 41 && S.footprints_lane_group == 59 && S.nnz == 61);
        CHECK(bits_of(S.max_quality) == 47 && bits_of(S.percentile) == 53);
        CHECK(S.pairs == 1009 && S.nnz_pre == 1013);
        // slots no field reads change no field
        unsigned long long c[C_N_STATS]; memcpy(c, primes, sizeof(c));
        c[C_SURV] = 0xDEADBEEFCAFEull; c[C_PASS] = ~0ull;
        mvs_dc_stats T; memset(&T, 0, sizeof(T));
        T.pairs = 1009; T.nnz_pre = 1013;
        dc_stats_from_counters(c, 59, 61, &T);
        CHECK(memcmp(&S, &T, sizeof(S)) == 0);
    }
    // ---- sums over ranges: 64 bits, and only the summed slots ----
    {
        unsigned long long sum[C_N_STATS] = {0}, block[C_N_STATS];
        for (int k = 0; k < C_N_STATS; ++k) block[k] = 0xFFFFFFF0ull + (unsigned)k;   // what one range can count, about
        const int n = 40;
        for (int r = 0; r < n; ++r) dc_counters_add(sum, block);
        for (int k = 0; k < C_N_SUMMED; ++k) CHECK(sum[k] == (unsigned long long)n * (0xFFFFFFF0ull + (unsigned)k) && sum[k] > (1ull << 36));
        CHECK(sum[C_MAX_Q_BITS] == 0 && sum[C_PCTL_BITS] == 0);                 // the report words are no counts
        mvs_dc_stats S; memset(&S, 0, sizeof(S));
        dc_stats_from_counters(sum, 3ull << 33, 5ull << 32, &S);
        CHECK(S.cull_backface == 40ull * 0xFFFFFFF0ull && S.ray_leaf_rounds == 40ull * (0xFFFFFFF0ull + 13));
        CHECK(S.ray_tris == 16ull * 40ull * (0xFFFFFFF0ull + 9) && S.ray_tris > (1ull << 41));
        CHECK(S.footprints_lane_group == (3ull << 33) && S.nnz == (5ull << 32));
    }
    // ---- max_quality / percentile from their bit patterns ----
    {
        const float vals[] = {0.0f, 1e-42f /* a denormal */, 1e30f, 0.7315f};
        CHECK(bits_of(vals[1]) != 0 && bits_of(vals[1]) < 0x00800000u);
        for (float mq : vals) for (float pc : vals) {
            unsigned long long c[C_N_STATS] = {0};
            c[C_MAX_Q_BITS] = bits_of(mq); c[C_PCTL_BITS] = bits_of(pc);
            mvs_dc_stats S; memset(&S, 0xAB, sizeof(S));
            dc_stats_from_counters(c, 0, 0, &S);
            CHECK(same_bits(S.max_quality, mq) && same_bits(S.percentile, pc));
        }
    }
    printf("ok\n");
    return 0;
}
