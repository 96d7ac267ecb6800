// Geometry of a multi-scalar multiplication: the window width and bucket sets of an MSM (msm_shape), and every grid, block, LDS
// size, stride and workspace size of its counting sort (msm_sort_geom) and of its accumulation and fold (msm_run_geom).  ONE
// definition, plain C++ (no device code): msm_prepare and msm_run_tables (msm_host.cuh, group.cuh) ask here, `ensure` and launch;
// tests/host/msm_geom.cpp holds it to the formulas written out on their own and prints msm_shape for tests/size_ladder.py's model.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace zk {
typedef uint32_t u32;
typedef uint64_t u64;

// ------------------------------------------------------------------ constants
static constexpr int MSM_MAX_C = 17;         // widest window: 2^16 buckets, which the sort takes in two halves of MSM_SORT_MAX_KH counters
static constexpr int MSM_AUTO_MAX_C = 17;    // widest window chosen automatically (resident tables)
static constexpr int MSM_ADHOC_MAX_C = 16;   // ... and without a table (a bucket set per window: the fold grows with every bucket)
static constexpr u32 MSM_SORT_MAX_KH = 1u << 15;   // counters of one sort workgroup's LDS histogram (128 KiB)
// launch constants of kernels_msm.cuh (the kernels are written against these names; what each one buys is told where it is used)
static constexpr int MSM_MAX_TABLES = 3;                  // base tables one launch serves (A, B1 and L of a proof share the sort of the assignment)
// work-items of a sort workgroup (one workgroup per CU: its histogram takes up to 128 KiB of LDS); 1024 measured the same as
// 512 (profiles/r3e_sort_workgroup_ab.txt)
#ifndef ZK_SORT_THREADS
#define ZK_SORT_THREADS 512
#endif
static constexpr u32 MSM_COARSE_BITS = 8;                 // keys per coarse bin = 256 (a window narrower than 9 bits takes k_msm_place)
static constexpr u32 MSM_FINE_TILE = 2048;                // pairs per workgroup of the fine pass (8 per work-item)
static constexpr int MSM_TILE_SCAN_THREADS = 256;
static constexpr u32 SCAN_ONE_THREADS = 256, SCAN_ONE_PER = 16, SCAN_ONE_MAX = 1u << 17;   // the scan of up to SCAN_ONE_MAX counters in ONE workgroup
static constexpr int SCAN_THREADS = 256;                  // ... and of more: one workgroup per chunk of SCAN_CHUNK counters
static constexpr int SCAN_PER_THREAD = 16;
static constexpr int SCAN_CHUNK = SCAN_THREADS * SCAN_PER_THREAD;
static constexpr u32 MSM_HEAVY_CHUNKS = 64;               // runs the partials of a heavy bucket are cut into (k_msm_heavy_reduce)
static constexpr unsigned MSM_HEAVY_THREADS = 64;         // work-items per workgroup of k_msm_heavy_reduce

// ------------------------------------------------------------------ tunables
// The MSM's tunables (zkhip_ctx_tune; the environment variables give their initial values, read ONCE when the context is created)
struct MsmKnobs {
    int cus = 256;            // compute units of the device: sizes the accumulation launch (one slice per resident work-item)
    int msm_c_env = 0;        // window width of the tables built / ad-hoc MSMs run from now on (0 = automatic)
    int skip_inf_mode = 0;    // which accumulation kernel meets bases at infinity how: 0 per table (MsmShape::skip_inf), 1 lanes always sit them out, 2 always the vote
    int msm_sets = 0;         // bucket sets of the tables built from now on: 1 = every window multiple, 2 = every second ... (0 = what fits the device)
    int msm_waves = 0;        // accumulation waves per SIMD (0 = per point type)
    u32 msm_lanes = 0;        // slices of the sorted list (0 = one per resident work-item)
    u32 msm_min_slice = 8;    // finest cut of the sorted list
    bool heavy_runs = true;   // k_msm_heavy_reduce before the fold (ZKHIP_MSM_HEAVY_RUNS=0: the row's workgroup sums a heavy bucket alone)
    int fold_hg = 32;         // shares a column of rows is cut into in k_msm_fold_cols (a power of two <= 256; ZKHIP_FOLD_HG): 128 rows = 4 serial additions +
                              // 5 tree levels instead of 16 + 3 at 8 (the fold is a chain of dependent additions: Poseidon BLS12-381 8.95 -> 7.85 ms single)
    bool fold_scan = true;    // scan form of the last fold step (else double-and-add)
    int msm_fused_waves = 0;  // accumulation waves per SIMD of the launch over A, B1 and L (zkhip_ctx::fuse_z; 0 = per point type)
    int msm_g1_waves = 0, msm_g2_waves = 0;   // slices per SIMD lane of a single-table G1 / G2 accumulation (0 = per point type)
    u32 sort_wgs = 256;       // workgroups of a counting-sort pass (chunks x windows): fewer = longer runs per (workgroup, bucket)
};

// one launch: grid, block and dynamic LDS bytes
struct MsmLaunch {
    u32 gx = 1, gy = 1, gz = 1, bx = 1, by = 1;
    size_t lds = 0;
};
static inline u32 msm_blocks(u64 n, u32 threads) { return (u32)((n + threads - 1) / threads); }

// ------------------------------------------------------------------ shape
struct MsmShape {
    u64 n;
    int c, W;
    u32 K;          // buckets per set = 2^(c-1)
    u32 sets;       // bucket sets: 1 when the bases carry every window multiple (all windows share one set), W without a table, in
                    // between for keys too large for W levels (window j: bucket set j % sets, table level j / sets)
    u32 levels;     // table levels the sorted entries refer to: ceil(W / sets) (1 without a table)
    u32 nkeys;      // sets * K
    u32 Lw, H;      // fold geometry: K = H rows of Lw buckets
    static constexpr u32 ndig = 2;   // digits of the fold: column and row of the bucket index
    int level_bits() const { return c * (int)sets; }   // level t of a table holds 2^(level_bits t) P
    bool skip_inf = true;   // which accumulation kernel: lanes sit out bases at infinity (tables that hold many: kernels_msm.cuh
                            // k_msm_accum SKIP_INF), or the rare one goes through the general code (tables that hold next to none)
    u32 nsums() const { return ndig * sets; }   // the fold leaves one sum per digit and bucket set: msm_combine adds them
};
// `table`: the bases carry precomputed window multiples 2^(c j) P (resident keys); otherwise one bucket set per window.
// `knobs` (may be null): its msm_c_env, when set, is the width; `force_c` goes before both.
static inline MsmShape msm_shape(const MsmKnobs* knobs, u64 n, int scalar_bits, bool table, int force_c = 0, int force_sets = 0) {
    MsmShape s;
    s.n = n;
    int lg = 0;
    for (u64 x = std::max<u64>(n, 1); x >>= 1;) ++lg;      // floor(log2 n)
    if (table) {
        // one fold per MSM whatever c is, so c only trades additions (n * W) against buckets (2^(c-1)): the fewest windows the
        // widest admissible width gives (a few points per bucket at least), and of the widths with that many windows the
        // narrowest — 254-bit scalars: 15 windows of 17 bits instead of 16 of 16 (6 % fewer additions in all five MSMs for twice
        // the buckets); 255-bit scalars need 16 windows either way and stay at 16 bits
        const int cmax = std::max(2, std::min(MSM_AUTO_MAX_C, lg + 1));
        const int Wmin = (scalar_bits + 1 + cmax - 1) / cmax;
        s.c = cmax;
        while (s.c > 2 && (scalar_bits + 1 + (s.c - 1) - 1) / (s.c - 1) == Wmin) --s.c;
    } else {
        // Window width: about log2(n) - 5 (measured optimum at 2^20: 15), but never one that leaves the top window
        // with only a few significant bits — its handful of buckets would each receive a large share of all points
        // (same-address atomics in the sort, one bucket spread over thousands of slices).
        const int want = std::max(2, std::min(MSM_ADHOC_MAX_C, lg - 5));
        s.c = want;
        for (int d = 0; d <= 14; ++d) {
            bool found = false;
            for (int cand : {want + d, want - d}) {
                if (cand < 2 || cand > MSM_ADHOC_MAX_C) continue;
                const int W = (scalar_bits + 1 + cand - 1) / cand;
                const int top_bits = scalar_bits + 1 - (W - 1) * cand;
                if (top_bits >= cand || (n >> (top_bits - 1)) <= 4096) { s.c = cand; found = true; break; }   // <= 4096 points per top bucket
            }
            if (found) break;
        }
    }
    if (knobs && knobs->msm_c_env) s.c = knobs->msm_c_env;
    if (force_c) s.c = force_c;
    s.c = std::min(s.c, MSM_MAX_C);
    s.W = (scalar_bits + 1 + s.c - 1) / s.c;
    s.K = 1u << (s.c - 1);
    s.sets = table ? (u32)std::max(1, std::min(force_sets ? force_sets : 1, s.W)) : (u32)s.W;
    s.levels = ((u32)s.W + s.sets - 1) / s.sets;
    s.nkeys = s.sets * s.K;
    s.Lw = std::min<u32>(s.K, 256);
    s.H = s.K / s.Lw;
    return s;
}
static inline MsmShape with_inf(MsmShape sh, bool many) { sh.skip_inf = many; return sh; }

// ------------------------------------------------------------------ digits + counting sort (msm_prepare)
// exclusive scan of nk counters in three kernels (k_scan_local / _chunks / _add): one workgroup per chunk of SCAN_CHUNK
struct MsmScanGeom {
    u32 nchunks;
    size_t off_bytes, chunk_sum_bytes, grand_bytes;
    MsmLaunch local, chunks, add;
};
static inline MsmScanGeom msm_scan_geom(u64 nk) {
    MsmScanGeom g;
    g.nchunks = msm_blocks(nk, SCAN_CHUNK);
    g.off_bytes = (nk + 1) * 4;                            // off[nk] = the sum
    g.chunk_sum_bytes = (size_t)g.nchunks * 4;
    g.grand_bytes = 4;
    g.local.gx = g.nchunks, g.local.bx = SCAN_THREADS;
    g.chunks.bx = SCAN_THREADS;
    g.add.gx = msm_blocks(nk + 1, 256), g.add.bx = 256;
    return g;
}
struct MsmSortGeom {
    // one workgroup of the count / place passes per (chunk of scalars, window, half): a window of more than 16 bits has more
    // buckets than one histogram holds, so its workgroups come in `halves`, each reading the chunk's digits and keeping the ones of
    // its own range of `kh` buckets
    u32 kh, halves;
    u64 sort_chunks, chunk;          // chunks of `chunk` scalars
    bool two_level;                  // placement: coarse bins of 2^MSM_COARSE_BITS keys, then tiles inside them (else k_msm_place)
    u32 nbins;                       // coarse bins over every bucket set
    bool scan_one;                   // the counters fit the one-workgroup scan (else three kernels, and k_msm_tile_offsets if two_level)
    u64 c_chunk;                     // scalars per workgroup of the coarse pass
    // bytes of MsmSort's buffers (0: this pass does not use it)
    size_t dig_bytes, sorted_bytes, cnt_bytes, cursor_bytes, ccur_bytes, tile_off_bytes, pairs_bytes, off_bytes, chunk_sum_bytes, grand_bytes;
    MsmLaunch digits, zero, count, place, scan_one_launch, tile_offsets, part_coarse, part_fine;   // (count and place: the same shape)
    MsmScanGeom scan;
};
static inline MsmSortGeom msm_sort_geom(const MsmShape& sh, u32 sort_wgs) {
    MsmSortGeom g;
    const u64 nk = sh.nkeys, entries = sh.n * (u64)sh.W;
    g.kh = std::min(sh.K, MSM_SORT_MAX_KH), g.halves = sh.K / g.kh;
    // chunks several times larger than a window's bucket count keep the global atomics (one per touched bucket per workgroup)
    // well below one per digit
    const u64 want_chunks = g.halves > 1 ? std::max<u64>(1, sort_wgs / (sh.W * g.halves)) : std::max<u64>(1, (sort_wgs + sh.W - 1) / sh.W);
    const u64 max_chunks = std::max<u64>(1, sh.n / (2 * (u64)g.kh));
    g.sort_chunks = std::min(want_chunks, max_chunks);
    g.chunk = (sh.n + g.sort_chunks - 1) / g.sort_chunks;
    g.two_level = sh.K >= (1u << MSM_COARSE_BITS) && sh.K <= (1u << 16);
    g.nbins = (u32)(nk >> MSM_COARSE_BITS);
    g.scan_one = nk <= SCAN_ONE_MAX;
    g.scan = msm_scan_geom(nk);
    g.dig_bytes = g.sorted_bytes = entries * 4;
    g.cnt_bytes = g.cursor_bytes = nk * 4;
    g.ccur_bytes = g.two_level ? (size_t)g.nbins * 4 : 0;
    g.tile_off_bytes = g.two_level ? ((size_t)g.nbins + 1) * 4 : 0;
    g.pairs_bytes = g.two_level ? std::max<u64>(entries, 1) * 8 : 0;
    g.off_bytes = g.scan.off_bytes;
    g.chunk_sum_bytes = g.scan_one ? 0 : g.scan.chunk_sum_bytes;
    g.grand_bytes = g.scan_one ? 0 : g.scan.grand_bytes;
    g.digits.gx = msm_blocks(sh.n, 256), g.digits.bx = 256;
    g.zero.gx = msm_blocks(nk, 256), g.zero.bx = 256;
    g.count.gx = (u32)g.sort_chunks, g.count.gy = (u32)sh.W, g.count.gz = g.halves, g.count.bx = ZK_SORT_THREADS, g.count.lds = (size_t)g.kh * 4;
    g.place = g.count;
    g.scan_one_launch.bx = SCAN_ONE_THREADS;
    g.tile_offsets.bx = MSM_TILE_SCAN_THREADS;
    // ~1024 workgroups of the coarse pass (1 KiB of LDS each: they share CUs with anything), chunks of at least 4096 scalars
    const u64 c_chunks = std::max<u64>(1, std::min<u64>((1024 + sh.W - 1) / sh.W, (sh.n + 4095) / 4096));
    g.c_chunk = (sh.n + c_chunks - 1) / c_chunks;
    g.part_coarse.gx = (u32)c_chunks, g.part_coarse.gy = (u32)sh.W, g.part_coarse.bx = 256;
    g.part_fine.gx = (u32)(entries / MSM_FINE_TILE + g.nbins), g.part_fine.bx = 256;      // the most tiles the bins can be cut into
    return g;
}

// ------------------------------------------------------------------ accumulation + fold (msm_run_tables)
struct MsmCut { u32 nlanes, min_slice; u32 table_len; };   // table_len: entries of a base table (levels x points), for the checked build
// what the arithmetic needs of a point type (group.cuh fills it from MsmTuning<F>)
struct MsmPoint {
    bool is_ext;                  // G2
    int slice_wpe, fused_wpe;     // slices per SIMD lane of a launch over one table / over the tables that share a list
    size_t xyzz_bytes;            // sizeof(Xyzz<F>), F the unsaturated field the kernels run on
    size_t xyzz_sat_bytes;        // sizeof(Xyzz<FS>), the saturated form the sums leave in
    size_t accum_lds;             // dynamic LDS of one accumulation workgroup
};
struct MsmRunGeom {
    int wpe;                      // slices per SIMD lane
    u32 nlanes;                   // slices of the sorted list
    MsmCut cut;
    u64 partial_stride;           // slot of (key, lane) = key + lane: collision free
    size_t heavy_bytes, lane_key_bytes, partial_bytes, bucket_bytes, rows_bytes, cols_bytes;   // MsmLane's buffers
    size_t sums_bytes;            // one table's sums, saturated
    bool skip_inf;                // which accumulation kernel
    bool heavy_reduce;            // k_msm_heavy_reduce runs
    u32 HG, CW;                   // k_msm_fold_cols: work-item (lo, hg) of a workgroup of CW columns adds H / HG rows serially
    bool final_scan;              // k_msm_fold_final_scan (one workgroup per digit), else k_msm_fold_final (double-and-add, both digits)
    MsmLaunch lane_keys, find_heavy, accum, heavy, fold_rows, fold_cols, fold_final;
};
static inline MsmRunGeom msm_run_geom(const MsmShape& sh, int nt, const MsmPoint& pt, const MsmKnobs& k) {
    MsmRunGeom g;
    // one slice of the sorted list per work-item the machine holds (never finer than msm_min_slice entries; the slices may
    // outnumber the work-items the kernel's registers let the machine hold).  msm_waves goes before everything; else the tables that
    // share a list have their own figure, shared between them, and a single table its group's
    g.wpe = k.msm_waves;
    if (!g.wpe && nt > 1) g.wpe = std::max(1, k.msm_fused_waves ? k.msm_fused_waves : pt.fused_wpe);
    if (!g.wpe) { const int own = pt.is_ext ? k.msm_g2_waves : k.msm_g1_waves; g.wpe = own ? own : pt.slice_wpe; }
    const u64 entries = sh.n * (u64)sh.W;
    const u64 machine = k.msm_lanes ? (u64)k.msm_lanes : (u64)k.cus * 4 * 64 * g.wpe / (nt > 1 && !k.msm_waves ? nt : 1);
    g.nlanes = (u32)std::max<u64>(1, std::min<u64>(machine, (entries + k.msm_min_slice - 1) / k.msm_min_slice));
    g.cut = MsmCut{g.nlanes, k.msm_min_slice, (u32)std::min<u64>(sh.n * (u64)sh.levels, 0x7fffffffu)};
    g.partial_stride = (u64)sh.nkeys + g.nlanes;
    g.heavy_bytes = ((size_t)sh.nkeys + 1) * 4;            // [0] = count, [1..] = keys
    g.lane_key_bytes = (size_t)g.nlanes * 4;
    g.partial_bytes = (size_t)nt * g.partial_stride * pt.xyzz_bytes;
    g.bucket_bytes = (size_t)nt * sh.nkeys * pt.xyzz_bytes;
    g.rows_bytes = (size_t)nt * sh.sets * sh.H * pt.xyzz_bytes;
    g.cols_bytes = (size_t)nt * sh.sets * sh.Lw * pt.xyzz_bytes;
    g.sums_bytes = (size_t)sh.nsums() * pt.xyzz_sat_bytes;
    g.skip_inf = k.skip_inf_mode == 1 || (k.skip_inf_mode == 0 && sh.skip_inf);
    g.heavy_reduce = k.heavy_runs;
    g.lane_keys.gx = msm_blocks(g.nlanes, 256), g.lane_keys.bx = 256;
    g.find_heavy.gx = msm_blocks(sh.nkeys, 256), g.find_heavy.bx = 256;
    g.accum.gx = msm_blocks(g.nlanes, 256), g.accum.gy = (u32)nt, g.accum.bx = 256, g.accum.lds = pt.accum_lds;
    g.heavy.gx = MSM_HEAVY_CHUNKS, g.heavy.gy = (u32)nt, g.heavy.bx = MSM_HEAVY_THREADS, g.heavy.lds = (size_t)MSM_HEAVY_THREADS * pt.xyzz_bytes;
    // one workgroup per (row, bucket set): Lw work-items
    g.fold_rows.gx = sh.H, g.fold_rows.gy = sh.sets, g.fold_rows.gz = (u32)nt, g.fold_rows.bx = sh.Lw, g.fold_rows.lds = (size_t)sh.Lw * pt.xyzz_bytes;
    // column sums of the K = H x Lw buckets of a set
    g.HG = std::max<u32>(1, std::min<u32>((u32)k.fold_hg, sh.H)), g.CW = std::min<u32>(sh.Lw, 256 / g.HG);
    g.fold_cols.gx = sh.Lw / g.CW, g.fold_cols.gy = sh.sets, g.fold_cols.gz = (u32)nt, g.fold_cols.bx = g.CW, g.fold_cols.by = g.HG;
    g.fold_cols.lds = (size_t)g.CW * g.HG * pt.xyzz_bytes;
    // the scan form of the last fold step: one workgroup of <= 256 work-items per digit (columns: Lw long, rows: H long); the
    // double-and-add form (two digits in one workgroup of Lw work-items) is the fallback.  Either leaves one sum per digit and bucket set.
    const u32 TS = std::max<u32>(64, std::max(sh.Lw, sh.H));
    g.final_scan = k.fold_scan && TS <= 256;
    if (g.final_scan) g.fold_final.gx = sh.sets, g.fold_final.gy = (u32)nt, g.fold_final.gz = sh.ndig, g.fold_final.bx = TS;
    else g.fold_final.gx = sh.sets, g.fold_final.gy = (u32)nt, g.fold_final.bx = std::max<u32>(64, sh.Lw);
    g.fold_final.lds = (size_t)g.fold_final.bx * pt.xyzz_bytes;
    return g;
}

// ------------------------------------------------------------------ resident tables: what fits the device
// What one proof slot is reckoned to allocate beside a key's tables: the digits and sorted lists of up to three sorts, the transform
// vectors, scalars, and the partial / bucket arrays of five MSMs plus the transient of the table construction.  An ESTIMATE made
// before any MSM has run, kept as it is (how many bucket sets a large key gets depends on it): it counts six workspaces of
// K + 2^19 points of 288 bytes each whatever the point type, where msm_run_geom sizes `partial` at nt * (nkeys + nlanes) points.
static inline u64 msm_slot_bytes(u64 z_n, u64 h_n, u64 N, int W, u32 K) {
    return (2 * z_n + h_n) * (u64)W * 16 + 4 * N * 32 + (z_n + 2) * 64 + 6 * ((u64)K + (1u << 19)) * 288 + ((u64)1 << 29);
}
// Bucket sets of the MSMs over z and over h: every s-th window multiple is in the tables.  Doubled from `start` until the tables
// `need(sets)` fit `budget` or both counts have reached `stop`; a doubled count never passes `cap`.
struct MsmSets { int z, h; };
template <class Need>
static inline MsmSets msm_pick_sets(MsmSets start, MsmSets cap, MsmSets stop, u64 budget, Need need) {
    MsmSets s = start;
    while (need(s) > budget && (s.z < stop.z || s.h < stop.h)) {
        s.z = std::min(2 * s.z, cap.z);
        s.h = std::min(2 * s.h, cap.h);
    }
    return s;
}

}  // namespace zk
