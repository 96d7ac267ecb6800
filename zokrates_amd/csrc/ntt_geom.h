// Geometry of a transform: how a domain of 2^logN splits into passes, the tile a workgroup of each pass stages, and the launch
// shape of one pass over a span of the domain.  ONE definition, plain C++ (no device code): get_plan and the pass launchers
// (ntt_host.cuh) take every grid, block and LDS size from here, tests/host/ntt_geom.cpp holds it to the formulas written out on
// their own and prints it for tests/size_ladder.py's model.
//
// A span is (ShardGeom, member k) of ntt_shard.h: strip k for the outer cols pass, range k for every other pass.  The whole domain
// is the span G = 1, k = 0: one strip of all Nb columns, one range of all N1 outer indices, origins 0.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ntt_shard.h"

namespace zk {

// LDS slots of one staged sequence of n elements: one pad per 32, one more so that sequences start on different banks
// (kernels_ntt.cuh: k_ntt_cols and k_ntt_rows lay their tiles out by the same rule)
constexpr int ntt_seq_stride(int n) { return n + (n >> 5) + 1; }

struct NttGeom {
    int log1 = 0, log2 = 0, log3 = 0;   // N = N1 * N2 * N3: cols pass over N1, (three passes, log3 > 0: cols pass over N2 inside every N2 x N3 block,) rows pass over the last factor
    uint64_t N = 1;
    uint32_t N1 = 1, N2 = 1, N3 = 1, M = 1;   // M = max(N1, N2, N3): root tables hold w_M^j, j < M; N3 = 1 for one or two passes
    uint64_t Nb = 1;                    // N2 * N3: the block of one outer index
    int C_cols = 1, R_rows = 1, threads_cols = 64, threads_rows = 64;
    size_t smem_cols = 0, smem_rows = 0;
    int C_mid = 1, threads_mid = 64;    // the middle pass of three: columns per workgroup, work-items
    size_t smem_mid = 0;
    int last_log() const { return log3 > 0 ? log3 : log2; }   // the rows pass's sequences
    // every tile divides what its pass runs over, and the outer indices of a middle pass fit grid.z
    bool launchable() const { return Nb % (uint64_t)C_cols == 0 && (N >> last_log()) % (uint64_t)R_rows == 0 && N3 % (uint32_t)C_mid == 0 && (log3 == 0 || N1 <= 65535); }
};

// a workgroup stages `nseq` sequences of n elements as nine limb planes
inline size_t ntt_tile_smem(uint32_t nseq, uint32_t n) { return (size_t)9 * nseq * ntt_seq_stride((int)n) * 4; }
inline int ntt_tile_threads(uint64_t butterflies) { return (int)std::min<uint64_t>(512, std::max<uint64_t>(64, (butterflies + 63) / 64 * 64)); }

// One pass up to 2^single_max, two passes (N1 x N2) up to 2^(2 max_sublog), three (N1 x N2 x N3) beyond (logN <= 3 max_sublog).
// A workgroup stages a tile of elements as nine limb planes (36 B + padding per element): tiles of 1024 elements (38 KiB) let four
// workgroups share a CU, so that one loads while another computes; a cols tile needs >= `ccols` columns (2: 64-byte rows in HBM).
inline NttGeom ntt_geom(int logN, int single_max, int max_sublog, uint32_t ccols) {
    NttGeom p;
    if (logN <= single_max && logN <= max_sublog) { p.log1 = 0; p.log2 = logN; p.log3 = 0; }
    else if (logN <= 2 * max_sublog) { p.log1 = logN / 2; p.log2 = logN - p.log1; p.log3 = 0; }
    else { p.log1 = logN / 3; p.log2 = (logN - p.log1) / 2; p.log3 = logN - p.log1 - p.log2; }
    p.N = (uint64_t)1 << logN;
    p.N1 = 1u << p.log1, p.N2 = 1u << p.log2, p.N3 = 1u << p.log3;
    p.Nb = (uint64_t)p.N2 * p.N3;
    p.M = std::max(p.N1, std::max(p.N2, p.N3));
    const uint32_t last = 1u << p.last_log();
    const uint64_t nrows = p.N / last;
    const uint32_t tile_rows = std::max<uint32_t>(last, (uint32_t)std::min<uint64_t>(p.N, 1024));
    p.R_rows = p.log1 == 0 ? 1 : (int)std::max<uint64_t>(1, std::min<uint64_t>(nrows, tile_rows / last));
    auto cols_per_wg = [&](uint64_t ncols, uint32_t n) { return (int)std::max<uint64_t>(1, std::min<uint64_t>(ncols, std::max<uint32_t>(ccols, 1024 / std::max<uint32_t>(n, 1)))); };
    p.C_cols = cols_per_wg(p.Nb, p.N1);
    p.smem_cols = ntt_tile_smem((uint32_t)p.C_cols, p.N1);
    p.smem_rows = ntt_tile_smem((uint32_t)p.R_rows, last);
    p.threads_cols = ntt_tile_threads((uint64_t)p.C_cols * p.N1 / 4);
    p.threads_rows = ntt_tile_threads((uint64_t)p.R_rows * last / 4);
    if (p.log3 > 0) {
        p.C_mid = cols_per_wg(p.N3, p.N2);
        p.smem_mid = ntt_tile_smem((uint32_t)p.C_mid, p.N2);
        p.threads_mid = ntt_tile_threads((uint64_t)p.C_mid * p.N2 / 4);
    }
    return p;
}
inline ShardGeom ntt_whole(const NttGeom& p) { return ntt_shard_geom(p.N1, p.Nb, 1); }

enum NttPass { NTT_COLS, NTT_MID, NTT_ROWS };
struct NttLaunch {
    uint32_t grid_x, grid_z;   // (grid.y: the vectors of the launch)
    int threads;
    size_t smem;
    int nseq;                  // sequences per workgroup: columns (cols, mid) or rows
    uint64_t offset;           // first element of the span in the vector
};
// The plan's kernels over strip k (cols) or range k (mid, rows) of the full-length vector: a pointer offset, a smaller grid, a tile
// that fits — columns per workgroup <= the strip's width, rows per workgroup <= the rows of the range.
inline NttLaunch ntt_pass_shape(const NttGeom& p, NttPass pass, const ShardGeom& g, uint32_t k) {
    if (pass == NTT_MID) return {p.N3 / (uint32_t)p.C_mid, g.rows, p.threads_mid, p.smem_mid, p.C_mid, g.range_origin(k)};
    const bool cols = pass == NTT_COLS;
    const uint32_t n = cols ? p.N1 : 1u << p.last_log();                                                        // length of a sequence
    const uint64_t have = cols ? g.W : g.range_len() / n;                                                       // sequences of the span
    const uint32_t nseq = (uint32_t)std::min<uint64_t>((uint64_t)(cols ? p.C_cols : p.R_rows), have);           // the tile that fits
    return {(uint32_t)(have / nseq), 1, ntt_tile_threads((uint64_t)nseq * n / 4), ntt_tile_smem(nseq, n), (int)nseq, cols ? g.strip_origin(k) : g.range_origin(k)};
}

}  // namespace zk
