// The launch geometry of the transforms (zokrates_amd/csrc/ntt_geom.h), on the CPU under ASan + UBSan.  For every domain size,
// every setting of the three knobs that shape a plan (ntt_max_sublog 2 .. 11, ntt_single_max_log 0 .. 11, ntt_cols 1 and 2):
//   * the plan (split, tiles, work-items, LDS bytes) against the rules written out here on their own;
//   * WHOLE: the shape of each pass over the whole domain (the span G = 1) is the launch a single context has always made —
//     cols grid (Nb / C_cols, nvec) with threads_cols and smem_cols; mid grid (N3 / C_mid, nvec, N1); rows grid ((N >> lg) / R_rows,
//     nvec) — at offset 0;
//   * SHARDED: for G = 2, 4, 8 and every member k of what shards, the shape over strip k / range k: Cw = min(C_cols, W) columns
//     and R = min(R_rows, rows of the range) rows per workgroup, grid.z = the range's outer indices, the origins as offsets; Cw | W
//     and R | nrows, so that the workgroups of a launch cover the span exactly and none runs past it.
// Prints the plan of every case as one JSON line (keys of tests/size_ladder.py ntt_plan): tests/test_size_ladder.py holds the
// Python model to it.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "ntt_geom.h"

using namespace zk;

// the slots of a staged sequence as k_ntt_cols and k_ntt_rows compute them (kernels_ntt.cuh: SS = n + (n >> 5) + 1)
constexpr bool seq_stride_is_the_kernels(int upto) {
    for (int n = 1; n <= upto; ++n)
        if (ntt_seq_stride(n) != n + (n >> 5) + 1) return false;
    return true;
}
static_assert(seq_stride_is_the_kernels(2048), "ntt_seq_stride differs from the stride the kernels lay their tiles out by");

static int failures = 0;
static int logN, single_max, sub;
static uint32_t ccols, G, k;
#define CHECK(cond)                                                                                                      \
    do {                                                                                                                 \
        if (!(cond) && ++failures <= 20)                                                                                 \
            fprintf(stderr, "FAILED %s (line %d): logN %d single_max %d sub %d ccols %u G %u k %u\n", #cond, __LINE__, logN, single_max, sub, ccols, G, k); \
    } while (0)

// the rules, in this file's own words
static uint64_t smem_of(uint64_t nseq, uint64_t n) { return 9 * nseq * (n + (n >> 5) + 1) * 4; }
static int threads_of(uint64_t butterflies) { return (int)std::min<uint64_t>(512, std::max<uint64_t>(64, (butterflies + 63) / 64 * 64)); }
static uint64_t cols_of(uint64_t ncols, uint64_t n) { return std::max<uint64_t>(1, std::min<uint64_t>(ncols, std::max<uint64_t>(ccols, 1024 / std::max<uint64_t>(n, 1)))); }

static bool same(const NttLaunch& L, uint64_t gx, uint64_t gz, int threads, uint64_t smem, uint64_t nseq, uint64_t off) {
    return L.grid_x == gx && L.grid_z == gz && L.threads == threads && L.smem == smem && (uint64_t)L.nseq == nseq && L.offset == off;
}

int main() {
    long cases = 0, sharded = 0;
    for (sub = 2; sub <= 11; ++sub)
        for (logN = 0; logN <= std::min(3 * sub, 47); ++logN)
            for (single_max = 0; single_max <= 11; ++single_max)
                for (uint32_t cc : {1u, 2u}) {
                    ccols = cc; G = 1; k = 0;
                    ++cases;
                    int l1, l2, l3;
                    if (logN <= single_max && logN <= sub) { l1 = 0; l2 = logN; l3 = 0; }
                    else if (logN <= 2 * sub) { l1 = logN / 2; l2 = logN - l1; l3 = 0; }
                    else { l1 = logN / 3; l2 = (logN - l1) / 2; l3 = logN - l1 - l2; }
                    const uint64_t N = (uint64_t)1 << logN, N1 = (uint64_t)1 << l1, N2 = (uint64_t)1 << l2, N3 = (uint64_t)1 << l3, Nb = N2 * N3;
                    const int lg = l3 > 0 ? l3 : l2;
                    const uint64_t last = (uint64_t)1 << lg, nrows = N >> lg;
                    const uint64_t R = l1 == 0 ? 1 : std::max<uint64_t>(1, std::min<uint64_t>(nrows, std::max<uint64_t>(last, std::min<uint64_t>(N, 1024)) / last));
                    const uint64_t Cc = cols_of(Nb, N1), Cm = l3 > 0 ? cols_of(N3, N2) : 1;
                    const int t_cols = threads_of(Cc * N1 / 4), t_rows = threads_of(R * last / 4), t_mid = l3 > 0 ? threads_of(Cm * N2 / 4) : 64;
                    const uint64_t s_cols = smem_of(Cc, N1), s_rows = smem_of(R, last), s_mid = l3 > 0 ? smem_of(Cm, N2) : 0;

                    const NttGeom p = ntt_geom(logN, single_max, sub, ccols);
                    CHECK(p.log1 == l1 && p.log2 == l2 && p.log3 == l3 && p.N == N && p.N1 == N1 && p.N2 == N2 && p.N3 == N3 && p.Nb == Nb);
                    CHECK(p.M == std::max(N1, std::max(N2, N3)) && p.last_log() == lg);
                    CHECK((uint64_t)p.C_cols == Cc && (uint64_t)p.R_rows == R && (uint64_t)p.C_mid == Cm);
                    CHECK(p.threads_cols == t_cols && p.threads_rows == t_rows && p.threads_mid == t_mid);
                    CHECK(p.smem_cols == s_cols && p.smem_rows == s_rows && p.smem_mid == s_mid);
                    CHECK(p.launchable() && Nb % Cc == 0 && nrows % R == 0 && N3 % Cm == 0);
                    CHECK(std::max(s_cols, std::max(s_rows, s_mid)) <= 160 * 1024);      // the LDS of a gfx950 workgroup

                    // the whole domain: what a single context launches
                    const ShardGeom w = ntt_whole(p);
                    CHECK(w.G == 1 && w.W == Nb && w.rows == N1 && w.N == N && w.strip_origin(0) == 0 && w.range_origin(0) == 0 && w.range_len() == N);
                    CHECK(!ntt_shardable(l1, (uint32_t)N1, Nb, 1));
                    CHECK(same(ntt_pass_shape(p, NTT_COLS, w, 0), Nb / Cc, 1, t_cols, s_cols, Cc, 0));
                    if (l3 > 0) CHECK(same(ntt_pass_shape(p, NTT_MID, w, 0), N3 / Cm, N1, t_mid, s_mid, Cm, 0));
                    CHECK(same(ntt_pass_shape(p, NTT_ROWS, w, 0), (N >> lg) / R, 1, t_rows, s_rows, R, 0));

                    printf("{\"single_max\": %d, \"sub\": %d, \"ccols\": %u, \"logN\": %d, \"log1\": %d, \"log2\": %d, \"log3\": %d, \"passes\": %d, \"split\": %d, "
                           "\"R_rows\": %d, \"C_cols\": %d, \"threads_cols\": %d, \"threads_rows\": %d, \"smem_cols\": %zu, \"smem_rows\": %zu",
                           single_max, sub, ccols, logN, p.log1, p.log2, p.log3, 1 + (p.log1 > 0) + (p.log3 > 0), p.log1 | (p.log3 << 8), p.R_rows, p.C_cols,
                           p.threads_cols, p.threads_rows, p.smem_cols, p.smem_rows);
                    if (p.log3 > 0) printf(", \"C_mid\": %d, \"threads_mid\": %d, \"smem_mid\": %zu", p.C_mid, p.threads_mid, p.smem_mid);
                    printf("}\n");

                    // strips and ranges
                    for (uint32_t members : {2u, 4u, 8u}) {
                        G = members; k = 0;
                        if (!ntt_shardable(l1, (uint32_t)N1, Nb, G)) continue;
                        ++sharded;
                        const ShardGeom g = ntt_shard_geom((uint32_t)N1, Nb, G);
                        const uint64_t W = Nb / G, rows = N1 / G;
                        const uint64_t Cw = std::min<uint64_t>(Cc, W), rn = (rows * Nb) >> lg, Rr = std::min<uint64_t>(R, rn);
                        CHECK(g.W == W && g.rows == rows && W % Cw == 0 && rn % Rr == 0);
                        for (k = 0; k < G; ++k) {
                            const NttLaunch c = ntt_pass_shape(p, NTT_COLS, g, k), r = ntt_pass_shape(p, NTT_ROWS, g, k);
                            CHECK(same(c, W / Cw, 1, threads_of(Cw * N1 / 4), smem_of(Cw, N1), Cw, g.strip_origin(k)) && c.offset == (uint64_t)k * W);
                            CHECK(same(r, rn / Rr, 1, threads_of(Rr * last / 4), smem_of(Rr, last), Rr, g.range_origin(k)) && r.offset == (uint64_t)k * rows * Nb);
                            // the workgroups of a launch cover the span exactly: the last one ends where the strip / the range does
                            CHECK((uint64_t)c.grid_x * c.nseq == W && c.offset + W <= Nb && c.smem <= s_cols);
                            CHECK((uint64_t)r.grid_x * r.nseq * last == g.range_len() && r.offset + g.range_len() <= N && r.smem <= s_rows);
                            if (l3 > 0) {
                                const NttLaunch m = ntt_pass_shape(p, NTT_MID, g, k);
                                CHECK(same(m, N3 / Cm, rows, t_mid, s_mid, Cm, g.range_origin(k)));
                                CHECK((uint64_t)m.grid_x * m.nseq == N3 && m.grid_z * Nb == g.range_len());
                            }
                        }
                    }
                }
    fprintf(stderr, "%ld plans, %ld sharded, %d failures\n", cases, sharded, failures);
    return failures ? 1 : 0;
}
