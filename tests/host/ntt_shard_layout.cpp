// The geometry of a transform sharded across the members of a zkhip_multi (zokrates_amd/csrc/ntt_shard.h), on the CPU under
// ASan + UBSan: for every split (log1, log2, log3) of every domain up to 2^14 and every member count, the predicate against the
// stated rule, and for what shards: the G^2 blocks tile the N1 x Nb matrix exactly once, block (r, c) lies in range r and strip c,
// strips and ranges are disjoint and complete, and the staging slots of one, two and three vectors neither overlap nor leave their
// buffer.  Every index is used on a buffer of exactly the stated size, so an index past it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ntt_shard.h"

using namespace zk;

static int failures = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            if (++failures <= 20) printf("FAILED %s (line %d): log %d %d %d G %u\n", #cond, __LINE__, log1, log2, log3, G); \
        }                                                                                      \
    } while (0)

static bool all_ones(const std::vector<uint8_t>& v) {
    for (uint8_t x : v)
        if (x != 1) return false;
    return true;
}

int main() {
    long shardable = 0, refused = 0;
    for (int log1 = 0; log1 <= 14; ++log1)
        for (int log2 = 0; log1 + log2 <= 14; ++log2)
            for (int log3 = 0; log1 + log2 + log3 <= 14; ++log3) {
                const uint32_t N1 = 1u << log1;
                const uint64_t Nb = (uint64_t)1 << (log2 + log3), N = (uint64_t)N1 * Nb;
                for (uint32_t G : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 12u, 15u, 16u, 17u, 24u, 31u, 32u, 33u, 64u, 96u, 128u}) {
                    // the stated rule, written out on its own
                    bool pow2 = false;
                    for (uint32_t p = 2; p <= 128; p *= 2) pow2 = pow2 || p == G;
                    const bool want = pow2 && log1 > 0 && G <= N1 && 2ull * G <= Nb;
                    CHECK(ntt_shardable(log1, N1, Nb, G) == want);
                    if (!want) { ++refused; continue; }
                    ++shardable;
                    const ShardGeom g = ntt_shard_geom(N1, Nb, G);
                    CHECK(g.N == N && (uint64_t)g.W * G == Nb && g.rows * G == N1 && g.block == (uint64_t)g.rows * g.W && g.W >= 2 && g.rows >= 1);
                    CHECK(g.range_len() * G == N && g.range_len() % Nb == 0);
                    // blocks: each element exactly once, inside its range and its strip
                    std::vector<uint8_t> cover(N, 0);
                    bool inside = true;
                    for (uint32_t r = 0; r < G; ++r)
                        for (uint32_t c = 0; c < G; ++c)
                            for (uint32_t row = 0; row < g.rows; ++row)
                                for (uint32_t col = 0; col < g.W; ++col) {
                                    const uint64_t i = g.block_origin(r, c) + (uint64_t)row * Nb + col;
                                    ++cover[i];
                                    inside = inside && i >= g.range_origin(r) && i < g.range_origin(r) + g.range_len() && i % Nb >= g.strip_origin(c) &&
                                             i % Nb < g.strip_origin(c) + g.W;
                                }
                    CHECK(all_ones(cover) && inside);
                    // strips
                    std::vector<uint8_t> strips(N, 0);
                    for (uint32_t k = 0; k < G; ++k)
                        for (uint32_t row = 0; row < N1; ++row)
                            for (uint32_t col = 0; col < g.W; ++col) ++strips[g.strip_origin(k) + (uint64_t)row * Nb + col];
                    CHECK(all_ones(strips));
                    // ranges: whole blocks of Nb, starting on a multiple of Nb
                    std::vector<uint8_t> ranges(N, 0);
                    for (uint32_t k = 0; k < G; ++k) {
                        CHECK(g.range_origin(k) % Nb == 0);
                        for (uint64_t i = 0; i < g.range_len(); ++i) ++ranges[g.range_origin(k) + i];
                    }
                    CHECK(all_ones(ranges));
                    // staging
                    for (uint32_t nvec = 1; nvec <= 3; ++nvec) {
                        CHECK(g.staging_len(nvec) == (uint64_t)nvec * N / G);      // a member sends and receives 1/G of every vector (its own slot included)
                        std::vector<uint8_t> st(g.staging_len(nvec), 0);
                        for (uint32_t v = 0; v < nvec; ++v)
                            for (uint32_t peer = 0; peer < G; ++peer)
                                for (uint64_t i = 0; i < g.block; ++i) ++st[g.slot_origin(v, peer) + i];
                        CHECK(all_ones(st));
                    }
                }
            }
    printf("%ld shardable geometries, %ld refused, %d failures\n", shardable, refused, failures);
    return failures ? 1 : 0;
}
