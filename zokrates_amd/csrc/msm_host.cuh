// Host side of the multi-scalar multiplications: the digit / counting-sort pass (msm_prepare), the memory a key's tables may take,
// the accumulation and fold launchers' declarations (defined per point type in group.cuh) and the host's last step (msm_combine).
// Every size, grid, block and stride comes from msm_geom.h: the functions here ask the geometry, `ensure` and launch.  Included by
// core.cuh behind the context; no kernel lives here (kernels_msm.cuh).
#pragma once

namespace zk {

static inline dim3 msm_grid(const MsmLaunch& l) { return dim3(l.gx, l.gy, l.gz); }
static inline dim3 msm_block(const MsmLaunch& l) { return dim3(l.bx, l.by); }
#define MSM_LAUNCH(kernel, shape, stream, ...) ZK_LAUNCH(kernel, msm_grid(shape), msm_block(shape), (shape).lds, stream, __VA_ARGS__)

// Device memory the window-multiple tables of a key may take: 60 % of what is free now, less what the proofs themselves will
// allocate later beside them (msm_slot_bytes per proof slot) and the transient of the table construction (msm_table_levels:
// < 1 GiB).  Several contexts sharing one device each see the same "free" figure: the margin is what keeps the first batch prove
// from failing where the key load succeeded.
static inline u64 msm_table_budget(const zkhip_ctx* ctx, u64 z_n, u64 h_n, u64 N, int W, u32 K) {
    size_t free_b = 0, total_b = 0;
    dev_mem_info(&free_b, &total_b);
    const u64 later = (u64)std::max(1, ctx->nslots) * msm_slot_bytes(z_n, h_n, N, W, K) + ((u64)1 << 30);
    const u64 budget = (u64)((ctx->tenants > 1 ? 0.5 : 0.6) * (double)free_b) / (u64)std::max(1, ctx->tenants);
    return budget > later ? budget - later : 0;
}
// exclusive scan of the counters in three kernels (cnt -> off, off[nk] = their sum, also left in *grand)
static inline void scan_u32(Stream s, const MsmScanGeom& g, const DBuf& cnt, DBuf& off, u64 nk, DBuf& chunk_sum, DBuf& grand) {
    off.ensure(g.off_bytes);
    chunk_sum.ensure(g.chunk_sum_bytes);
    grand.ensure(g.grand_bytes);
    MSM_LAUNCH(k_scan_local, g.local, s, ptr<u32>(cnt), ptr<u32>(off), ptr<u32>(chunk_sum), nk);
    MSM_LAUNCH(k_scan_chunks, g.chunks, s, ptr<u32>(chunk_sum), g.nchunks, ptr<u32>(grand));
    MSM_LAUNCH(k_scan_add, g.add, s, ptr<u32>(off), ptr<u32>(chunk_sum), nk, ptr<u32>(grand));
}
// digits + counting sort on the main stream; leaves so.off / so.sorted describing every bucket's point list.
// level_stride: distance between two levels of the base tables this sort will be paired with (table mode), else 0.
// `keep`: bitmap of the scalars that take part (null: all); `wm_of`: a sort of the SAME scalars (same shape) whose digits are reused
static inline void msm_prepare(zkhip_ctx* ctx, Stream s, MsmSort& so, const u32* d_scalars, const MsmShape& sh, u64 level_stride,
                               const u32* keep = nullptr, const MsmSort* wm_of = nullptr) {
    const u32 nk = sh.nkeys;
    require(sh.n * (u64)sh.W < ((u64)1 << 32) - sh.nkeys, ZKHIP_ERR_BAD_ARG, "MSM too large for 32-bit sort offsets");
    require(level_stride * (u64)sh.levels < ((u64)1 << 31) && sh.n < ((u64)1 << 31), ZKHIP_ERR_BAD_ARG, "MSM too large for 31-bit table indices");
    const MsmSortGeom g = msm_sort_geom(sh, ctx->msm.sort_wgs);
    if (!wm_of) so.dig.ensure(g.dig_bytes);
    so.sorted.ensure(g.sorted_bytes);
    so.cnt.ensure(g.cnt_bytes);
    so.cursor.ensure(g.cursor_bytes);
    so.ccur.ensure(g.ccur_bytes);
    so.tile_off.ensure(g.tile_off_bytes);
    // the counters of the passes below start from zero: cleared by the digit kernel on its way (a sort that borrows another's digits:
    // by a launch of its own)
    const MsmZero zero{{ptr<u32>(so.cnt), ptr<u32>(so.cursor), g.two_level ? ptr<u32>(so.ccur) : nullptr}, {nk, nk, g.two_level ? g.nbins : 0u}};
    if (!wm_of) MSM_LAUNCH(k_msm_digits, g.digits, s, d_scalars, sh.n, sh.c, sh.W, ptr<u32>(so.dig), zero);
    else MSM_LAUNCH(k_msm_zero, g.zero, s, zero);
    const u32* wm = wm_of ? ptr<u32>(wm_of->dig) : ptr<u32>(so.dig);
    lds_opt_in(ctx, (const void*)k_msm_count);
    lds_opt_in(ctx, (const void*)k_msm_place);
    MSM_LAUNCH(k_msm_count, g.count, s, wm, sh.n, sh.c, sh.W, g.chunk, sh.sets, g.kh, ptr<u32>(so.cnt), keep);
    if (g.scan_one) {
        so.off.ensure(g.off_bytes);
        MSM_LAUNCH(k_scan_one, g.scan_one_launch, s, ptr<u32>(so.cnt), ptr<u32>(so.off), nk, g.two_level ? ptr<u32>(so.tile_off) : (u32*)nullptr, g.nbins);
    } else {
        scan_u32(s, g.scan, so.cnt, so.off, nk, so.chunk_sum, so.grand);
        if (g.two_level) MSM_LAUNCH(k_msm_tile_offsets, g.tile_offsets, s, ptr<u32>(so.off), g.nbins, ptr<u32>(so.tile_off));
    }
    if (g.two_level) {
        so.pairs.ensure(g.pairs_bytes);
        MSM_LAUNCH(k_msm_part_coarse, g.part_coarse, s, wm, sh.n, sh.c, sh.W, g.c_chunk, sh.sets, level_stride, ptr<u32>(so.off), ptr<u32>(so.ccur),
                   (unsigned long long*)so.pairs.p, keep);
        MSM_LAUNCH(k_msm_part_fine, g.part_fine, s, (const unsigned long long*)so.pairs.p, ptr<u32>(so.off), ptr<u32>(so.tile_off), g.nbins, ptr<u32>(so.cursor),
                   ptr<u32>(so.sorted));
    } else {
        MSM_LAUNCH(k_msm_place, g.place, s, wm, sh.n, sh.c, sh.W, g.chunk, sh.sets, g.kh, level_stride, ptr<u32>(so.off), ptr<u32>(so.cursor), ptr<u32>(so.sorted), keep);
    }
    event_record(so.ready, s);
}

// bucket accumulation + fold for one base table; the bucket sets' weighted sums land in d_window_sums[0..nsums()), two per set.
// Defined in group.cuh and instantiated once per (curve, group) in its own translation unit (bn254_g1.hip, ...):
// the elliptic-curve kernels are by far the most expensive code to compile.
// Runs on lane.stream after so.ready; lane.done is recorded behind the last kernel.
// `d_table` holds packed affine points (AffPacked, level-major when it carries window multiples); the sums come back in
// the saturated Montgomery form.
// `h_window_sums` (may be null): the pinned host mirror of d_window_sums — the lane copies its sums out itself, behind its fold and
// before `done`, so that the host can take each MSM's result as it arrives (Prover::finish) instead of all of them after the last
template <class F>
void msm_run(zkhip_ctx* ctx, MsmLane& lane, const MsmSort& so, const void* d_table, const MsmShape& sh, Xyzz<F>* d_window_sums,
             Event ev_begin, Event ev_end, Event accum_after = nullptr, Xyzz<F>* h_window_sums = nullptr);
template <class F>
void msm_run_tables(zkhip_ctx* ctx, MsmLane& lane, const MsmSort& so, const void* const* d_tables, int nt, const MsmShape& sh, Xyzz<F>* d_window_sums,
                    u32 sum_stride, Event ev_begin, Event ev_end, Event accum_after, Xyzz<F>* h_window_sums = nullptr);
// affine points, saturated Montgomery form -> packed working form of the MSM kernels (level 0 of a table); on ctx->stream
template <class F>
void points_to_packed(zkhip_ctx* ctx, const Aff<F>* d_in, void* d_out, u64 n);
// levels 1 .. L-1 (2^(bits j) P) behind a level 0 of `count` points; synchronises ctx->stream
template <class F>
void msm_table_levels(zkhip_ctx* ctx, void* d_table, u64 count, int bits, int L);
template <class F>
u64 count_infinite(zkhip_ctx* ctx, const void* d_table, u64 count);
template <class F>
void mark_finite(zkhip_ctx* ctx, const void* d_table, u64 count, u32* d_bitmap);
template <class F> static constexpr size_t packed_point_bytes() { return sizeof(AffPacked<typename Unsat<F>::type>); }

// the MSM's value from its bucket-set sums: the single sum of a table MSM, else the host Horner step sum_j 2^(c j) S_j
template <class F>
static Xyzz<F> msm_combine(const Xyzz<F>* ws, const MsmShape& sh) {
    auto set_sum = [&](int j) {                      // one sum per fold digit
        Xyzz<F> t = ws[sh.ndig * j];
        for (u32 d = 1; d < sh.ndig; ++d) t = xyzz_add(t, ws[sh.ndig * j + d]);
        return t;
    };
    if (sh.sets == 1) return set_sum(0);
    Xyzz<F> acc = Xyzz<F>::inf();
    for (int j = (int)sh.sets - 1; j >= 0; --j) {
        for (int i = 0; i < sh.c; ++i) acc = xyzz_dbl(acc);
        acc = xyzz_add(acc, set_sum(j));
    }
    return acc;
}

}  // namespace zk
