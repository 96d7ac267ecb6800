// The launch geometry of the multi-scalar multiplications (zokrates_amd/csrc/msm_geom.h), on the CPU under ASan + UBSan.  For the
// scalar widths of the three curves, with and without tables, n = 1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 up to 2^26, every forced width
// (and none), every forced number of bucket sets (and none):
//   * msm_shape against the rule written out here on its own;
//   * msm_sort_geom (sort_wgs 16, 256, 4096) against the arithmetic msm_prepare used to do between its launches;
//   * msm_run_geom against the arithmetic msm_run_tables used to do — the fold under every fold_hg / fold_scan / heavy_runs, one
//     to three tables and the G1 and G2 point types of every curve; the slicing under every wave knob at 0 and at its ends,
//     msm_lanes, msm_min_slice and 1 or 256 compute units;
//   * the invariants a launch must keep whatever the formulas say: no empty grid, grid y / z within 65535, blocks within the
//     kernels' launch bounds, dynamic LDS within 160 KiB, the fold's tiles covering K exactly, every byte size = elements x
//     element size;
//   * msm_pick_sets against the two doubling loops it replaced (key load, image import), copied here, over every budget from
//     nothing to "everything fits".
// Prints msm_shape of every (n, bits, table, force_c) as one JSON line (keys of tests/size_ladder.py msm_shape):
// tests/test_size_ladder.py holds the Python model to it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "msm_geom.h"

using namespace zk;

static int failures = 0;
static u64 n;
static int bits, force_c, force_sets;
static bool table;
static const char* what = "";
#define CHECK(cond)                                                                                                                          \
    do {                                                                                                                                     \
        if (!(cond) && ++failures <= 20)                                                                                                     \
            fprintf(stderr, "FAILED %s (line %d): n %llu bits %d table %d force_c %d force_sets %d %s\n", #cond, __LINE__, (unsigned long long)n, bits, \
                    (int)table, force_c, force_sets, what);                                                                                  \
    } while (0)

static u64 cdiv(u64 a, u64 b) { return (a + b - 1) / b; }
static bool launch_is(const MsmLaunch& l, u64 gx, u64 gy, u64 gz, u64 bx, u64 by, u64 lds) {
    return l.gx == gx && l.gy == gy && l.gz == gz && l.bx == bx && l.by == by && l.lds == lds;
}
// what every launch must keep: `bound` = the kernel's __launch_bounds__ (1024 where it has none)
static bool launchable(const MsmLaunch& l, u32 bound) {
    return l.gx >= 1 && l.gy >= 1 && l.gz >= 1 && l.gx <= 0x7fffffffu && l.gy <= 65535 && l.gz <= 65535 && l.bx >= 1 && l.by >= 1 && l.bx * l.by <= bound &&
           l.lds <= 160 * 1024;
}

// ---- the shape, in this file's own words
struct Shape { int c, W; u64 K, sets, levels, nkeys, Lw, H; };
static int windows(int c) { return (int)cdiv((u64)bits + 1, (u64)c); }
static Shape shape_rule(int knob_c) {
    int lg = 0;
    while (lg < 63 && ((u64)2 << lg) <= std::max<u64>(n, 1)) ++lg;
    int c;
    if (table) {
        const int cmax = std::max(2, std::min(17, lg + 1));
        c = cmax;
        for (int narrower = cmax - 1; narrower >= 2 && windows(narrower) == windows(cmax); --narrower) c = narrower;   // the narrowest with as few windows
    } else {
        const int want = std::max(2, std::min(16, lg - 5));
        c = want;
        bool found = false;
        for (int d = 0; d < 15 && !found; ++d)
            for (int cand : {want + d, want - d}) {
                if (cand < 2 || cand > 16) continue;
                const int top = bits + 1 - (windows(cand) - 1) * cand;      // significant bits of the top window
                if (top >= cand || (n >> (top - 1)) <= 4096) { c = cand; found = true; break; }
            }
    }
    if (knob_c) c = knob_c;
    if (force_c) c = force_c;
    c = std::min(c, 17);
    Shape s;
    s.c = c, s.W = windows(c), s.K = (u64)1 << (c - 1);
    s.sets = table ? (u64)std::max(1, std::min(force_sets ? force_sets : 1, s.W)) : (u64)s.W;
    s.levels = cdiv((u64)s.W, s.sets);
    s.nkeys = s.sets * s.K;
    s.Lw = std::min<u64>(s.K, 256), s.H = s.K / s.Lw;
    return s;
}

// ---- the sort
static void check_sort(const MsmShape& sh, const Shape& r, u32 wgs) {
    what = "sort";
    const MsmSortGeom g = msm_sort_geom(sh, wgs);
    const u64 entries = n * (u64)r.W, nk = r.nkeys;
    const u64 kh = r.K > 32768 ? 32768 : r.K, halves = r.K / kh;
    const u64 want = halves > 1 ? std::max<u64>(1, wgs / ((u64)r.W * halves)) : std::max<u64>(1, cdiv(wgs, (u64)r.W));
    const u64 chunks = std::min(want, std::max<u64>(1, n / (2 * kh))), chunk = cdiv(n, chunks);
    const bool two = r.K >= 256 && r.K <= 65536, one = nk <= ((u64)1 << 17);
    const u64 nbins = nk / 256;
    CHECK(g.kh == kh && g.halves == halves && halves * kh == r.K && (halves == 1 || halves == 2) && g.sort_chunks == chunks && g.chunk == chunk);
    CHECK(g.sort_chunks * g.chunk >= n && g.sort_chunks >= 1);
    CHECK(g.two_level == two && g.nbins == nbins && g.scan_one == one);
    // bytes = elements x element size
    CHECK(g.dig_bytes == entries * sizeof(u32) && g.sorted_bytes == entries * sizeof(u32) && g.cnt_bytes == nk * sizeof(u32) && g.cursor_bytes == nk * sizeof(u32));
    CHECK(g.ccur_bytes == (two ? nbins * sizeof(u32) : 0) && g.tile_off_bytes == (two ? (nbins + 1) * sizeof(u32) : 0));
    CHECK(g.pairs_bytes == (two ? std::max<u64>(entries, 1) * sizeof(u64) : 0) && g.off_bytes == (nk + 1) * sizeof(u32));
    const u64 scan_chunks = cdiv(nk, 256 * 16);
    CHECK(g.chunk_sum_bytes == (one ? 0 : scan_chunks * sizeof(u32)) && g.grand_bytes == (one ? 0 : sizeof(u32)));
    // launches
    CHECK(launch_is(g.digits, cdiv(n, 256), 1, 1, 256, 1, 0) && launch_is(g.zero, cdiv(nk, 256), 1, 1, 256, 1, 0));
    CHECK(launch_is(g.count, chunks, (u64)r.W, halves, 512, 1, kh * 4) && launch_is(g.place, chunks, (u64)r.W, halves, 512, 1, kh * 4));
    CHECK(launch_is(g.scan_one_launch, 1, 1, 1, 256, 1, 0) && launch_is(g.tile_offsets, 1, 1, 1, 256, 1, 0));
    CHECK(g.scan.nchunks == scan_chunks && g.scan.off_bytes == (nk + 1) * 4 && g.scan.chunk_sum_bytes == scan_chunks * 4 && g.scan.grand_bytes == 4);
    CHECK(launch_is(g.scan.local, scan_chunks, 1, 1, 256, 1, 0) && launch_is(g.scan.chunks, 1, 1, 1, 256, 1, 0) && launch_is(g.scan.add, cdiv(nk + 1, 256), 1, 1, 256, 1, 0));
    const u64 c_chunks = std::max<u64>(1, std::min<u64>(cdiv(1024, (u64)r.W), cdiv(n, 4096)));
    CHECK(g.c_chunk == cdiv(n, c_chunks) && launch_is(g.part_coarse, c_chunks, (u64)r.W, 1, 256, 1, 0) && c_chunks * g.c_chunk >= n);
    if (two) CHECK(launch_is(g.part_fine, entries / 2048 + nbins, 1, 1, 256, 1, 0) && launchable(g.part_fine, 256) && launchable(g.part_coarse, 256));
    CHECK(launchable(g.digits, 1024) && launchable(g.zero, 1024) && launchable(g.count, 512) && launchable(g.place, 512) && launchable(g.scan_one_launch, 256));
    CHECK(launchable(g.scan.local, 1024) && launchable(g.scan.chunks, 1024) && launchable(g.scan.add, 1024) && launchable(g.tile_offsets, 1024));
    CHECK(g.count.lds == (size_t)g.kh * sizeof(u32));      // the histogram: kh counters
}

// ---- accumulation and fold
struct Point { const char* name; MsmPoint pt; };
// (G2?, slices per SIMD lane single / fused, bytes of an XYZZ point in the 29- / 28-bit working form and saturated, LDS of the accumulation)
static const Point POINTS[] = {
    {"bn254 G1", {false, 4, 6, 4 * 9 * 4, 4 * 32, 0}},        {"bn254 G2", {true, 4, 4, 4 * 2 * 9 * 4, 4 * 64, 2 * 18 * 256 * 4}},
    {"bls12-381 G1", {false, 2, 3, 4 * 14 * 4, 4 * 48, 0}},   {"bls12-381 G2", {true, 1, 1, 4 * 2 * 14 * 4, 4 * 96, 0}},
    {"bls12-377 G1", {false, 2, 3, 4 * 14 * 4, 4 * 48, 0}},   {"bls12-377 G2", {true, 1, 1, 4 * 2 * 14 * 4, 4 * 96, 0}},
};
static void check_run(const MsmShape& sh, const Shape& r, int nt, const Point& p, const MsmKnobs& k) {
    what = p.name;
    const MsmPoint& pt = p.pt;
    const MsmRunGeom g = msm_run_geom(sh, nt, pt, k);
    const u64 entries = n * (u64)r.W, pb = pt.xyzz_bytes;
    // the slicing: which figure of waves holds, and among how many tables the machine is shared
    u64 wpe, share = 1;
    if (k.msm_waves) wpe = (u64)k.msm_waves;
    else if (nt > 1) wpe = (u64)std::max(1, k.msm_fused_waves ? k.msm_fused_waves : pt.fused_wpe), share = (u64)nt;
    else if (pt.is_ext) wpe = (u64)(k.msm_g2_waves ? k.msm_g2_waves : pt.slice_wpe);
    else wpe = (u64)(k.msm_g1_waves ? k.msm_g1_waves : pt.slice_wpe);
    const u64 machine = k.msm_lanes ? k.msm_lanes : (u64)k.cus * 256 * wpe / share;
    const u64 nlanes = std::max<u64>(1, std::min(machine, cdiv(entries, k.msm_min_slice)));
    CHECK((u64)g.wpe == wpe && g.nlanes == nlanes && g.cut.nlanes == nlanes && g.cut.min_slice == k.msm_min_slice);
    CHECK(g.cut.table_len == std::min<u64>(n * r.levels, 0x7fffffffu));
    CHECK(g.partial_stride == r.nkeys + nlanes);
    CHECK(g.heavy_bytes == (r.nkeys + 1) * sizeof(u32) && g.lane_key_bytes == nlanes * sizeof(u32));
    CHECK(g.partial_bytes == (u64)nt * (r.nkeys + nlanes) * pb && g.bucket_bytes == (u64)nt * r.nkeys * pb);
    CHECK(g.rows_bytes == (u64)nt * r.sets * r.H * pb && g.cols_bytes == (u64)nt * r.sets * r.Lw * pb && g.sums_bytes == 2 * r.sets * pt.xyzz_sat_bytes);
    CHECK(g.skip_inf == (k.skip_inf_mode == 1 || (k.skip_inf_mode == 0 && sh.skip_inf)) && g.heavy_reduce == k.heavy_runs);
    CHECK(launch_is(g.lane_keys, cdiv(nlanes, 256), 1, 1, 256, 1, 0) && launch_is(g.find_heavy, cdiv(r.nkeys, 256), 1, 1, 256, 1, 0));
    CHECK(launch_is(g.accum, cdiv(nlanes, 256), (u64)nt, 1, 256, 1, pt.accum_lds) && launch_is(g.heavy, 64, (u64)nt, 1, 64, 1, 64 * pb));
    CHECK(launch_is(g.fold_rows, r.H, r.sets, (u64)nt, r.Lw, 1, r.Lw * pb));
    // the columns: HG shares of the H rows (never more than there are rows), CW columns per workgroup
    const u64 HG = std::max<u64>(1, std::min<u64>((u64)k.fold_hg, r.H)), CW = std::min<u64>(r.Lw, 256 / HG);
    CHECK(g.HG == HG && g.CW == CW && launch_is(g.fold_cols, r.Lw / CW, r.sets, (u64)nt, CW, HG, CW * HG * pb));
    CHECK(HG * CW <= 256 && r.Lw % CW == 0 && r.H % HG == 0 && r.Lw * r.H == r.K && HG <= r.H);
    const u64 TS = std::max<u64>(64, std::max(r.Lw, r.H)), TF = std::max<u64>(64, r.Lw);
    const bool scan = k.fold_scan && TS <= 256;
    CHECK(g.final_scan == scan);
    if (scan) CHECK(launch_is(g.fold_final, r.sets, (u64)nt, 2, TS, 1, TS * pb) && TS <= 256 && TS >= r.Lw && TS >= r.H);
    else CHECK(launch_is(g.fold_final, r.sets, (u64)nt, 1, TF, 1, TF * pb) && TF >= r.Lw);
    CHECK(launchable(g.lane_keys, 1024) && launchable(g.find_heavy, 1024) && launchable(g.accum, 256) && launchable(g.heavy, 256));
    CHECK(launchable(g.fold_rows, 256) && launchable(g.fold_cols, 256) && launchable(g.fold_final, 256));
}

// ---- the bucket sets of a key: the two loops msm_pick_sets replaced, as they stood
static u64 wz, wh, pz, ph;      // windows of the MSMs over z / over h, bytes of one level of their tables
static u64 clamped(u64 sets, u64 W) { return std::max<u64>(1, std::min(sets, W)); }      // MsmShape::sets of a forced count
static u64 tables_need(u64 sz, u64 shh) { return pz * cdiv(wz, clamped(sz, wz)) + ph * cdiv(wh, clamped(shh, wh)); }
static int former_key_load(u64 budget) {
    int sets = 1;
    for (;;) {
        const u64 a_sets = clamped((u64)sets, wz);
        if (tables_need((u64)sets, (u64)sets) <= budget || (int)a_sets < sets) break;
        sets *= 2;
    }
    return sets;
}
static MsmSets former_image_import(int s_z, int s_h, u64 budget) {
    const int W_z = (int)wz, W_h = (int)wh;
    for (;;) {
        if (tables_need((u64)s_z, (u64)s_h) <= budget || (s_z >= W_z && s_h >= W_h)) break;
        s_z = std::min(2 * s_z, W_z);
        s_h = std::min(2 * s_h, W_h);
    }
    return {s_z, s_h};
}
static long check_pick_sets() {
    what = "pick_sets";
    long runs = 0;
    auto need = [](MsmSets s) { return tables_need((u64)s.z, (u64)s.h); };
    for (u64 a : {1, 2, 3, 15, 16, 17, 43, 64, 86, 128})
        for (u64 b : {1, 2, 3, 15, 16, 17, 43, 64, 86, 128})
            for (u64 sizes : {0, 1, 2}) {
                wz = a, wh = b, pz = sizes == 1 ? 7 : 1000, ph = sizes == 2 ? 7 : 900;
                std::set<u64> budgets = {0};
                for (u64 s = 1; s <= 256; s *= 2)
                    for (u64 t = 1; t <= 256; t *= 2) { const u64 v = tables_need(s, t); budgets.insert(v - 1), budgets.insert(v), budgets.insert(v + 1); }
                CHECK(*budgets.rbegin() > tables_need(1, 1));      // ... up to "everything fits"
                for (u64 budget : budgets) {
                    const int no_cap = 1 << 30;
                    const int got = msm_pick_sets({1, 1}, {no_cap, no_cap}, {(int)wz + 1, 0}, budget, need).z;
                    CHECK(got == former_key_load(budget));
                    ++runs;
                    for (int s_z : {1, 2, 3, 4, 16, 17, 255})
                        for (int s_h : {1, 2, 5, 16, 64, 255}) {
                            const MsmSets want = former_image_import(s_z, s_h, budget);
                            const MsmSets have = msm_pick_sets({s_z, s_h}, {(int)wz, (int)wh}, {(int)wz, (int)wh}, budget, need);
                            CHECK(have.z == want.z && have.h == want.h);
                            ++runs;
                        }
                }
            }
    return runs;
}

int main() {
    static_assert(MSM_MAX_C == 17 && MSM_AUTO_MAX_C == 17 && MSM_ADHOC_MAX_C == 16 && MSM_SORT_MAX_KH == 32768, "the widths");
    static_assert(MSM_COARSE_BITS == 8 && MSM_FINE_TILE == 2048 && SCAN_CHUNK == 4096 && SCAN_THREADS == 256 && SCAN_ONE_MAX == 131072 && SCAN_ONE_THREADS == 256, "sort constants");
    static_assert(MSM_TILE_SCAN_THREADS == 256 && MSM_HEAVY_CHUNKS == 64 && MSM_HEAVY_THREADS == 64 && MSM_MAX_TABLES == 3 && ZK_SORT_THREADS == 512, "launch constants");
    std::vector<u64> ns = {1, 2};      // (3 = 2^2 - 1)
    for (int k = 2; k <= 26; ++k)
        for (u64 v : {((u64)1 << k) - 1, (u64)1 << k, ((u64)1 << k) + 1}) ns.push_back(v);
    const MsmKnobs dflt;
    long cases = 0, sorts = 0, runs = 0;
    for (int b : {254, 255, 253})
        for (int t = 0; t < 2; ++t)
            for (u64 nn : ns)
                for (int fc = 0; fc <= 17; fc = fc ? fc + 1 : 2)
                    for (int fs = 0; fs <= (t ? 64 : 0); fs = fs ? 2 * fs : 1) {
                        bits = b, table = t != 0, n = nn, force_c = fc, force_sets = fs;
                        what = "shape";
                        const Shape r = shape_rule(0);
                        const MsmShape sh = msm_shape(nullptr, n, bits, table, force_c, force_sets);
                        CHECK(sh.n == n && sh.c == r.c && sh.W == r.W && sh.K == r.K && sh.sets == r.sets && sh.levels == r.levels && sh.nkeys == r.nkeys);
                        CHECK(sh.Lw == r.Lw && sh.H == r.H && (u64)sh.Lw * sh.H == sh.K && sh.nsums() == 2 * r.sets && sh.level_bits() == r.c * (int)r.sets && sh.skip_inf);
                        CHECK(sh.c >= 2 && sh.c <= 17 && sh.W * sh.c >= bits + 1 && (sh.W - 1) * sh.c < bits + 1 && sh.levels * sh.sets >= (u32)sh.W);
                        {   // the context's width goes before the automatic one and behind a forced one; no width set = no knobs
                            MsmKnobs kc;
                            const MsmShape same = msm_shape(&kc, n, bits, table, force_c, force_sets);
                            kc.msm_c_env = 5;
                            const MsmShape five = msm_shape(&kc, n, bits, table, force_c, force_sets);
                            CHECK(same.c == sh.c && same.sets == sh.sets && five.c == shape_rule(5).c && five.c == (force_c ? force_c : 5));
                        }
                        for (u32 wgs : {16u, 256u, 4096u}) { check_sort(sh, r, wgs); ++sorts; }
                        // the fold, under every knob that shapes it
                        for (const Point& p : POINTS)
                            for (int nt = 1; nt <= 3; ++nt)
                                for (int hg : {1, 32, 256})
                                    for (int fscan = 0; fscan < 2; ++fscan)
                                        for (int heavy = 0; heavy < 2; ++heavy) {
                                            MsmKnobs k;
                                            k.fold_hg = hg, k.fold_scan = fscan != 0, k.heavy_runs = heavy != 0;
                                            check_run(sh, r, nt, p, k);
                                            ++runs;
                                        }
                        for (int mode = 0; mode < 3; ++mode)
                            for (int many = 0; many < 2; ++many) {
                                MsmKnobs k;
                                k.skip_inf_mode = mode;
                                check_run(with_inf(sh, many != 0), r, 1, POINTS[mode], k);
                                ++runs;
                            }
                        // the slicing, under every knob that shapes it (it sees the shape as n x W entries and nothing else)
                        if (fs == 0 && fc == 0)
                            for (const Point& p : {POINTS[0], POINTS[1], POINTS[2], POINTS[3]})
                                for (int cus : {1, 256})
                                    for (int nt = 1; nt <= 3; ++nt)
                                        for (int waves : {0, 1, 8})
                                            for (int fused : {0, 1, 8})
                                                for (int g1 : {0, 1, 16})
                                                    for (int g2 : {0, 1, 16})
                                                        for (u32 lanes : {0u, 1u})
                                                            for (u32 min_slice : {1u, 8u, 1u << 20}) {
                                                                MsmKnobs k;
                                                                k.cus = cus, k.msm_waves = waves, k.msm_fused_waves = fused, k.msm_g1_waves = g1, k.msm_g2_waves = g2;
                                                                k.msm_lanes = lanes, k.msm_min_slice = min_slice;
                                                                check_run(sh, r, nt, p, k);
                                                                ++runs;
                                                            }
                        if (fs) continue;
                        ++cases;
                        const MsmSortGeom g = msm_sort_geom(sh, dflt.sort_wgs);
                        printf("{\"n\": %llu, \"bits\": %d, \"table\": %s, \"force_c\": %d, \"c\": %d, \"W\": %d, \"K\": %u, \"sets\": %u, \"halves\": %u, \"two_level\": %s, "
                               "\"Lw\": %u, \"H\": %u}\n",
                               (unsigned long long)n, bits, table ? "true" : "false", force_c, sh.c, sh.W, sh.K, sh.sets, g.halves, g.two_level ? "true" : "false", sh.Lw, sh.H);
                    }
    // the per-slot estimate of the budget: the expression msm_table_budget always used
    what = "slot bytes";
    for (u64 z : {(u64)0, (u64)5, (u64)1 << 20, (u64)1 << 26})
        for (u64 N : {(u64)1, (u64)1 << 20, (u64)1 << 28})
            for (int W : {15, 16, 128})
                for (u32 K : {2u, 1u << 15, 1u << 16})
                    CHECK(msm_slot_bytes(z, N, N, W, K) == (2 * z + N) * (u64)W * 16 + N * 128 + (z + 2) * 64 + ((u64)K + 524288) * 1728 + 536870912);
    const long picks = check_pick_sets();
    fprintf(stderr, "%ld sorts, %ld accumulation and fold launches, %ld choices of bucket sets; %ld cases, %d failures\n", sorts, runs, picks, cases, failures);
    return failures ? 1 : 0;
}
