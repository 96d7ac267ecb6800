// Host side of the transforms: the plan of a domain (tables and geometry), one launcher per pass over a span of the domain
// (ntt_geom.h: the whole domain is the span G = 1), the two transform kinds and the quotient's sequence built from them, the
// exchanges of a sharded transform, and the entry points that transform and nothing else.  Included by core.cuh behind the
// context; no kernel lives here (kernels_ntt.cuh).
#pragma once

namespace zk {

// ------------------------------------------------------------------ NTT plan
template <class C>
struct NttPlan : NttPlanBase, NttGeom {
    typedef typename C::Fr Fr;
    typedef Fu<typename Fr::Params> FrU;   // the passes' working form (kernels_ntt.cuh)
    int split() const { return log1 | (log3 << 8); }   // what the sigma order depends on besides N (zkhip_pk::ntt_log1, key images)
    // roots: 9-limb R'-form; tw (inter-pass twiddles, the inverse ones times 1/N... see get_plan), s_coset (g^i / N, sigma
    // order), s_cosetinv_canon (g^-i / N as plain integers: the Montgomery exit): packed, N entries each
    DBuf roots_fwd, roots_inv, tw_fwd, tw_inv, s_coset, s_cosetinv_canon;
    DBuf s_cexit;            // zinv / N as plain integers, N entries: exit factor of the transform that turns c's evaluations into
                             // its share zinv * c_i of the quotient's coefficients (canonical integers)
    DBuf tw2_fwd, tw2_inv;   // three passes: the twiddles inside a block, w_Nb^(k2 * j3), Nb entries
    DBuf plan1[2], plan2[2], plan3[2];   // twiddle plans of the N1-, N2- and N3-point sub-NTTs, [0] forward, [1] inverse (kernels_ntt.cuh)
    u32 plen1 = 0, plen2 = 0, plen3 = 0;
    Fr omega, omega_inv, n_inv, g, g_inv, zinv;   // saturated Montgomery form (host code, setup)
    Fr zinv_rp;                                   // zinv in R'-form (k_quotient)
    Fr k_to_rp, k_mont_to_rp;                     // canonical integer -> R'-form, saturated Montgomery -> R'-form (fe_mul by these)
};

template <class Fr>
static Fr host_root_of_unity(int two_adicity, u64 generator, int logN) {
    // GENERATOR^((r-1) >> S), then squared down to order 2^logN   (App. A.4)
    u32 e[Fr::N];
    u64 bw = 1;
    for (int i = 0; i < Fr::N; ++i) {
        u64 t = (u64)Fr::Params::mod(i) - bw;
        e[i] = (u32)t;
        bw = t >> 63;
    }
    for (int s = 0; s < two_adicity; ++s)
        for (int i = 0; i < Fr::N; ++i) e[i] = (e[i] >> 1) | (i + 1 < Fr::N ? e[i + 1] << 31 : 0);
    Fr root = fe_pow(fe_from_u64<typename Fr::Params>(generator), e, Fr::N);
    for (int i = logN; i < two_adicity; ++i) root = fe_sqr(root);
    return root;
}
// R' = 2^(29*9) as a canonical integer mod p: Fr::one() is the integer 2^256 mod p, doubled 5 more times.  fe_mul(x R, R') = x R';
// its Montgomery form takes a canonical integer there: fe_mul(x, R' R) = x R'.
template <class Fr>
static Fr rp_factor() {
    Fr rp = Fr::one();
    for (int i = 32 * Fr::N; i < Fu<typename Fr::Params>::B * Fu<typename Fr::Params>::N; ++i) rp = fe_add(rp, rp);
    return rp;
}

static constexpr int NTT_MAX_SUBLOG = 11;   // 2^11 x 32 B = 64 KiB per staged sequence

template <class C>
static NttPlan<C>* get_plan(zkhip_ctx* ctx, int logN) {
    typedef typename C::Fr Fr;
    for (auto& p : ctx->plans)
        if (p->curve == C::ID && p->logN == logN) return (NttPlan<C>*)p.get();
    const int sub = ctx->ntt_max_sublog;
    require(logN >= 0 && logN <= 3 * sub && logN <= C::TWO_ADICITY, ZKHIP_ERR_BAD_ARG,
            "domain size unsupported (log2 N must not exceed the field's two-adicity: 28 for bn128, 32 for bls12_381, 47 for bls12_377)");
    auto* pl = new NttPlan<C>();
    ctx->plans.emplace_back(pl);
    pl->curve = C::ID;
    pl->logN = logN;
    // the split and the launch geometry (ntt_geom.h).  The reference's radix-2 domain goes up to the field's two-adicity (ark-poly
    // Radix2EvaluationDomain), so does this one
    static_cast<NttGeom&>(*pl) = ntt_geom(logN, ctx->ntt_single_max, sub, (u32)ctx->ntt_cols);
    require(pl->launchable(), ZKHIP_ERR_BAD_ARG, "internal: NTT tile does not divide the domain, or its batch exceeds the grid");
    pl->omega = host_root_of_unity<Fr>(C::TWO_ADICITY, C::GENERATOR, logN);
    pl->omega_inv = fe_inv(pl->omega);
    pl->n_inv = fe_inv(fe_from_u64<typename Fr::Params>(pl->N));
    pl->g = fe_from_u64<typename Fr::Params>(C::GENERATOR);
    pl->g_inv = fe_inv(pl->g);
    pl->zinv = fe_inv(fe_sub(fe_pow_u64(pl->g, pl->N), Fr::one()));
    Stream s = ctx->stream;
    const unsigned T = 256;
    const Fr rp = rp_factor<Fr>();
    pl->k_mont_to_rp = rp;
    pl->k_to_rp = fe_to_mont(rp);
    pl->zinv_rp = fe_mul(pl->zinv, rp);
    typedef typename NttPlan<C>::FrU FrU;
    auto to_rp = [&](DBuf& buf, u64 count) {  // saturated Montgomery table -> packed R'-form, in place
        ZK_LAUNCH((k_mul_const<Fr>), dim3(blocks_for(count, T)), dim3(T), 0, s, ptr<Fr>(buf), ptr<Fr>(buf), count, rp);
    };
    // sub-NTT roots: w_M^j, j < M (the radix-4 butterflies use w^pos, w^2pos, w^3pos), as 9-limb R'-form values
    const Fr wM = fe_pow_u64(pl->omega, pl->N / pl->M);
    const u64 nroots = std::max<u64>(pl->M, 1);
    ctx->tmp.ensure(nroots * sizeof(Fr));
    for (int inv = 0; inv < 2; ++inv) {
        DBuf& dst = inv ? pl->roots_inv : pl->roots_fwd;
        dst.ensure(nroots * sizeof(FrU));
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(nroots, T)), dim3(T), 0, s, ptr<Fr>(ctx->tmp), inv ? fe_inv(wM) : wM, Fr::one(), nroots, 0u, 0u, 0, 1u);
        to_rp(ctx->tmp, nroots);
        ZK_LAUNCH((k_unpack_table<typename Fr::Params>), dim3(blocks_for(nroots, T)), dim3(T), 0, s, ptr<Fr>(ctx->tmp), ptr<FrU>(dst), nroots);
    }
    // the sub-NTTs' twiddle plans, gathered from the root tables
    {
        std::vector<u32> src;
        DBuf d_src;
        for (int which = 0; which < 3; ++which) {
            if (which == 2 && pl->log3 == 0) break;
            const int lg = which == 0 ? pl->log1 : which == 1 ? pl->log2 : pl->log3;
            const u32 plen = ntt_plan_len(lg);
            (which == 0 ? pl->plen1 : which == 1 ? pl->plen2 : pl->plen3) = plen;
            ntt_plan_exponents(lg, src);
            d_src.ensure(src.size() * 4);
            dev_h2d(d_src.p, src.data(), src.size() * 4, s);
            for (int inv = 0; inv < 2; ++inv) {
                DBuf& dst = which == 0 ? pl->plan1[inv] : which == 1 ? pl->plan2[inv] : pl->plan3[inv];
                dst.ensure((size_t)plen * NTT_PLAN_STRIDE * 4);
                ZK_LAUNCH((k_ntt_plan_gather<typename Fr::Params>), dim3(blocks_for(plen, T)), dim3(T), 0, s, ptr<FrU>(inv ? pl->roots_inv : pl->roots_fwd),
                          (int)(pl->M >> lg), ptr<u32>(d_src), plen, ptr<u32>(dst));
            }
            stream_sync(s);   // src is reused
        }
    }
    if (pl->log1 > 0) {
        // between the pass over N1 and what follows: w_N^(k1 * j), j < Nb the position inside the block of k1
        pl->tw_fwd.ensure(pl->N * sizeof(Fr));
        pl->tw_inv.ensure(pl->N * sizeof(Fr));
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(pl->N, T)), dim3(T), 0, s, ptr<Fr>(pl->tw_fwd), pl->omega, Fr::one(), pl->N, pl->N1, (u32)pl->Nb, 1, 1u);
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(pl->N, T)), dim3(T), 0, s, ptr<Fr>(pl->tw_inv), pl->omega_inv, Fr::one(), pl->N, pl->N1, (u32)pl->Nb, 1, 1u);
        to_rp(pl->tw_fwd, pl->N);
        to_rp(pl->tw_inv, pl->N);
    }
    if (pl->log3 > 0) {
        // inside a block: w_Nb^(k2 * j3), the two-pass rule once more (w_Nb = w_N^N1)
        const Fr wb = fe_pow_u64(pl->omega, pl->N1), wb_inv = fe_pow_u64(pl->omega_inv, pl->N1);
        pl->tw2_fwd.ensure(pl->Nb * sizeof(Fr));
        pl->tw2_inv.ensure(pl->Nb * sizeof(Fr));
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(pl->Nb, T)), dim3(T), 0, s, ptr<Fr>(pl->tw2_fwd), wb, Fr::one(), pl->Nb, pl->N2, pl->N3, 1, 1u);
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(pl->Nb, T)), dim3(T), 0, s, ptr<Fr>(pl->tw2_inv), wb_inv, Fr::one(), pl->Nb, pl->N2, pl->N3, 1, 1u);
        to_rp(pl->tw2_fwd, pl->Nb);
        to_rp(pl->tw2_inv, pl->Nb);
    }
    pl->s_coset.ensure(pl->N * sizeof(Fr));
    pl->s_cosetinv_canon.ensure(pl->N * sizeof(Fr));
    ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(pl->N, T)), dim3(T), 0, s, ptr<Fr>(pl->s_coset), pl->g, pl->n_inv, pl->N, pl->N1, pl->N2, 2, pl->N3);
    to_rp(pl->s_coset, pl->N);
    // plain integers: multiplying an R'-form value by them (R' Montgomery product) leaves the plain value
    ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(pl->N, T)), dim3(T), 0, s, ptr<Fr>(pl->s_cosetinv_canon), pl->g_inv, fe_from_mont(pl->n_inv), pl->N,
              pl->N1, pl->N2, 2, pl->N3);
    pl->s_cexit.ensure(pl->N * sizeof(Fr));
    ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(pl->N, T)), dim3(T), 0, s, ptr<Fr>(pl->s_cexit), Fr::one(), fe_from_mont(fe_mul(pl->n_inv, pl->zinv)), pl->N,
              0u, 0u, 0, 1u);
    lds_opt_in(ctx, (const void*)k_ntt_cols<typename Fr::Params>);
    lds_opt_in(ctx, (const void*)k_ntt_rows<typename Fr::Params>);
    stream_sync(s);
    return pl;
}

// ------------------------------------------------------------------ the passes over span (g, k) of the domain, and what is built of them
template <class C>
struct Transforms {
    typedef typename C::Fr Fr;
    // Member k of a sharded transform runs the outer pass on its strip of columns and every other pass on its range of rows
    // (ntt_shard.h); a single context runs them over ntt_whole(*pl), member 0.  `nvec` vectors of N elements, vec_stride elements
    // apart, go through one launch (grid.y).  `post` and `minus` tables as long as the vector move with the data, tables per block
    // (post_mask = Nb - 1) stay: a range starts on a multiple of Nb.
    // the pass over N1: columns of the N1 x Nb matrix
    static void ntt_cols(zkhip_ctx* ctx, NttPlan<C>* pl, const ShardGeom& g, u32 k, Fr* data, bool inverse, const Fr* post, int nvec,
                         u64 vec_stride, int canon = 0) {
        const NttLaunch L = ntt_pass_shape(*pl, NTT_COLS, g, k);
        ZK_LAUNCH((k_ntt_cols<typename Fr::Params>), dim3(L.grid_x, nvec), dim3(L.threads), L.smem, ctx->ws, data + L.offset, vec_stride, pl->log1, (u32)pl->Nb, L.nseq,
                  ptr<u32>(pl->plan1[inverse ? 1 : 0]), pl->plen1, post ? post + L.offset : post, canon, (const Fr*)nullptr, (u64)0, ~(u64)0, ctx->ntt_fuse_first);
    }
    // three passes only — the pass over N2: columns of the N2 x N3 matrix of every outer index (grid.z).  `post_mask`: Nb - 1 for
    // the per-block twiddles, all ones for a table as long as the vector.
    static void ntt_mid(zkhip_ctx* ctx, NttPlan<C>* pl, const ShardGeom& g, u32 k, Fr* data, bool inverse, const Fr* post, u64 post_mask,
                        int nvec, u64 vec_stride) {
        const NttLaunch L = ntt_pass_shape(*pl, NTT_MID, g, k);
        ZK_LAUNCH((k_ntt_cols<typename Fr::Params>), dim3(L.grid_x, nvec, L.grid_z), dim3(L.threads), L.smem, ctx->ws, data + L.offset, vec_stride, pl->log2, pl->N3,
                  L.nseq, ptr<u32>(pl->plan2[inverse ? 1 : 0]), pl->plen2, (post && post_mask == ~(u64)0) ? post + L.offset : post, 0, (const Fr*)nullptr, pl->Nb,
                  post_mask, ctx->ntt_fuse_first);
    }
    // the pass over the last factor: contiguous sequences
    static void ntt_rows(zkhip_ctx* ctx, NttPlan<C>* pl, const ShardGeom& g, u32 k, Fr* data, bool inverse, const Fr* post, int nvec,
                         u64 vec_stride, int canon = 0, const Fr* minus = nullptr, u64 post_mask = ~(u64)0) {
        const bool three = pl->log3 > 0;
        const NttLaunch L = ntt_pass_shape(*pl, NTT_ROWS, g, k);
        ZK_LAUNCH((k_ntt_rows<typename Fr::Params>), dim3(L.grid_x, nvec), dim3(L.threads), L.smem, ctx->ws, data + L.offset, vec_stride, pl->last_log(), L.nseq,
                  ptr<u32>((three ? pl->plan3 : pl->plan2)[inverse ? 1 : 0]), three ? pl->plen3 : pl->plen2, (post && post_mask == ~(u64)0) ? post + L.offset : post, canon,
                  minus ? minus + L.offset : minus, post_mask, ctx->ntt_fuse_first);
    }
    // natural order in -> sigma order out
    static void ntt_kind_a(zkhip_ctx* ctx, NttPlan<C>* pl, Fr* data, bool inverse, const Fr* final_post, int nvec = 1,
                           u64 vec_stride = 0, int canon = 0, const Fr* final_minus = nullptr) {
        const ShardGeom w = ntt_whole(*pl);
        if (pl->log1 > 0) ntt_cols(ctx, pl, w, 0, data, inverse, inverse ? ptr<Fr>(pl->tw_inv) : ptr<Fr>(pl->tw_fwd), nvec, vec_stride);
        if (pl->log3 > 0) ntt_mid(ctx, pl, w, 0, data, inverse, inverse ? ptr<Fr>(pl->tw2_inv) : ptr<Fr>(pl->tw2_fwd), pl->Nb - 1, nvec, vec_stride);
        ntt_rows(ctx, pl, w, 0, data, inverse, final_post, nvec, vec_stride, canon, final_minus);
    }
    // sigma order in -> natural order out
    static void ntt_kind_b(zkhip_ctx* ctx, NttPlan<C>* pl, Fr* data, bool inverse, const Fr* final_post, int nvec = 1,
                           u64 vec_stride = 0, int canon = 0) {
        const ShardGeom w = ntt_whole(*pl);
        if (pl->log3 > 0) {
            ntt_rows(ctx, pl, w, 0, data, inverse, inverse ? ptr<Fr>(pl->tw2_inv) : ptr<Fr>(pl->tw2_fwd), nvec, vec_stride, 0, nullptr, pl->Nb - 1);
            ntt_mid(ctx, pl, w, 0, data, inverse, inverse ? ptr<Fr>(pl->tw_inv) : ptr<Fr>(pl->tw_fwd), ~(u64)0, nvec, vec_stride);
            ntt_cols(ctx, pl, w, 0, data, inverse, final_post, nvec, vec_stride, canon);
        } else if (pl->log1 > 0) {
            ntt_rows(ctx, pl, w, 0, data, inverse, inverse ? ptr<Fr>(pl->tw_inv) : ptr<Fr>(pl->tw_fwd), nvec, vec_stride);
            ntt_cols(ctx, pl, w, 0, data, inverse, final_post, nvec, vec_stride, canon);
        } else {
            ntt_rows(ctx, pl, w, 0, data, inverse, final_post, nvec, vec_stride, canon);
        }
    }
    // The transforms around a quotient, on ctx->ws: `nvec` evaluation vectors at v (N apart) go to their coefficients and on to the
    // coset g<w> (natural order), where `pointwise(factor)` leaves their product over Z(g) in v.  Unbound, c only needs its
    // coefficients — ((ab - c)/Z)'s are coset_ifft(ab / Z) - c_coeffs / Z: the coset transform pair is the identity on the c term —
    // so c takes ONE inverse transform whose exit factor carries 1/(N Z) and leaves canonical integers, and the last transform
    // subtracts them where it stores h (sigma order).  A key bound to the system carries all that in its bases: the factor is a plain
    // integer, which takes the R'-form product out of the Montgomery domain (canonical integers, natural order).
    template <class Pointwise>
    static void ntt_quotient(zkhip_ctx* ctx, NttPlan<C>* pl, Fr* v, int nvec, Fr* c, bool bound, Pointwise pointwise) {
        const u64 stride = nvec > 1 ? pl->N : 0;
        ntt_kind_a(ctx, pl, v, true, ptr<Fr>(pl->s_coset), nvec, stride);                        // ifft, then * g^i   (coset shift)
        if (!bound) ntt_kind_a(ctx, pl, c, true, ptr<Fr>(pl->s_cexit), 1, 0, 1);                 // c: ifft * 1/(N Z), canonical integers, sigma order
        ntt_kind_b(ctx, pl, v, false, nullptr, nvec, stride);                                    // evaluations on g<w>
        pointwise(bound ? fe_from_mont(pl->zinv) : pl->zinv_rp);
        if (!bound) ntt_kind_a(ctx, pl, v, true, ptr<Fr>(pl->s_cosetinv_canon), 1, 0, 1, c);     // coset_ifft, canonical, minus c's share
    }

    // ------------------------------------------------------------------ transforms sharded across the members of a zkhip_multi
    // (ntt_shard.h: one all-to-all between the outer pass on a member's strip and the passes on its range)
    static bool shard_ok(const NttPlan<C>* pl, size_t G) { return ntt_shardable(pl->log1, pl->N1, pl->Nb, G); }
    // the staging of member `ctx` for exchanges of up to `nvec` vectors, its two events
    static void shard_state(zkhip_ctx* ctx, const ShardGeom& g, u32 nvec) {
        const size_t bytes = (size_t)g.staging_len(nvec) * 32;
        ctx->shard.send[0].ensure(bytes);
        ctx->shard.send[1].ensure(bytes);
        ctx->shard.recv.ensure(bytes);
        for (Event& e : ctx->shard.packed)
            if (!e) e = event_create();
    }
    static ShardMove shard_move_args(const ShardGeom& g, u32 k, u64 vec_stride, bool by_row, bool own) {
        ShardMove a;
        a.vec_stride = vec_stride;
        a.nb = g.Nb;
        a.G = g.G;
        a.me = k;
        a.rows = g.rows;
        a.log_w = ilog2_floor(g.W);
        a.by_row = by_row ? 1 : 0;
        a.own = own ? 1 : 0;
        return a;
    }
    static unsigned shard_move_blocks(const ShardGeom& g) { return (unsigned)std::min<u64>(1024, std::max<u64>(1, (2 * g.block + 255) / 256)); }
    // first half of an exchange: this member's G - 1 foreign blocks of `nvec` vectors into the staging set of this turn, `packed` behind
    static void shard_pack(zkhip_ctx* ctx, const ShardGeom& g, u32 k, const Fr* data, u32 nvec, u64 vec_stride, bool by_row) {
        zkhip_ctx::Shard& sh = ctx->shard;
        const unsigned set = sh.turn & 1u;
        ZK_LAUNCH((k_ntt_shard_pack<typename Fr::Params>), dim3(shard_move_blocks(g), nvec, g.G), dim3(256), 0, ctx->ws, data, ptr<Fr>(sh.send[set]),
                  shard_move_args(g, k, vec_stride, by_row, false));
        event_record(sh.packed[set], ctx->ws);
    }
    // second half, entered only when EVERY member has packed (the caller's two phases): the blocks the peers packed for this member
    // travel into its staging behind their `packed` events, one launch scatters them
    static void shard_fetch(zkhip_ctx* ctx, const ShardGeom& g, u32 k, Fr* data, u32 nvec, u64 vec_stride, bool by_row, zkhip_ctx* const* members) {
        zkhip_ctx::Shard& sh = ctx->shard;
        const unsigned set = sh.turn & 1u;
        for (u32 j = 0; j < g.G; ++j) {
            if (j == k) continue;
            event_sync(members[j]->shard.packed[set]);      // (the peer's stream, possibly on another device: waited for on the host, as split_fetch does)
            for (u32 v = 0; v < nvec; ++v)
                dev_copy_between(ptr<Fr>(sh.recv) + g.slot_origin(v, j), ctx->device, ptr<Fr>(members[j]->shard.send[set]) + g.slot_origin(v, k), members[j]->device,
                                 (size_t)g.block * sizeof(Fr), ctx->ws);
        }
        ZK_LAUNCH((k_ntt_shard_unpack<typename Fr::Params>), dim3(shard_move_blocks(g), nvec, g.G), dim3(256), 0, ctx->ws, data, ptr<Fr>(sh.recv),
                  shard_move_args(g, k, vec_stride, by_row, false));
        ++sh.turn;
    }

    // ------------------------------------------------------------------ entry points (CurveOps): transforms and nothing else
    // zkhip_ntt
    static void ntt_api(zkhip_ctx* ctx, u32 log_n, int dir, uint8_t* data) {
        NttPlan<C>* pl = get_plan<C>(ctx, (int)log_n);
        Stream s = ctx->stream;
        ctx->ws = s;
        const u64 N = pl->N;
        const unsigned T = 256, B = blocks_for(N, T);
        ctx->cur->va.ensure(N * sizeof(Fr));
        ctx->cur->vb.ensure(N * sizeof(Fr));
        ctx->cur->vc.ensure(N * sizeof(Fr));
        Fr *a = ptr<Fr>(ctx->cur->va), *b = ptr<Fr>(ctx->cur->vb), *t = ptr<Fr>(ctx->cur->vc);
        dev_h2d(a, data, N * 32, s);
        ZK_LAUNCH((k_mul_const<Fr>), dim3(B), dim3(T), 0, s, a, a, N, pl->k_to_rp);   // canonical -> R'-form
        const bool inverse = dir == 1 || dir == 3;
        if (dir == 2) {   // coset_fft: x_i * g^i first (a saturated-Montgomery factor keeps the R'-form)
            ZK_LAUNCH((k_pow_table<Fr>), dim3(B), dim3(T), 0, s, t, pl->g, Fr::one(), N, 0u, 0u, 0);
            ZK_LAUNCH((k_mul_table<Fr>), dim3(B), dim3(T), 0, s, a, t, a, N);
        }
        ntt_kind_a(ctx, pl, a, inverse, nullptr, 1, 0, 1);
        ZK_LAUNCH((k_sigma_permute<Fr>), dim3(B), dim3(T), 0, s, a, b, N, pl->N1, pl->N2, 1, pl->N3);
        if (inverse) {    // * 1/N (and g^-i for coset_ifft)
            ZK_LAUNCH((k_pow_table<Fr>), dim3(B), dim3(T), 0, s, t, dir == 3 ? pl->g_inv : Fr::one(), pl->n_inv, N, 0u, 0u, 0);
            ZK_LAUNCH((k_mul_table<Fr>), dim3(B), dim3(T), 0, s, b, t, b, N);
        }
        ZK_LAUNCH((k_from_rp<Fr>), dim3(B), dim3(T), 0, s, b, b, N);
        dev_d2h(data, b, N * 32, s);
        stream_sync(s);
        // A stand-alone transform of a very large domain leaves 8 N x 32 bytes behind (five factor tables of its plan, three work
        // vectors: 69 GiB at 2^28) that nothing else will use at that size: given back at once.  A prover at such a domain keeps its
        // plan (it is rebuilt in about a second if a transform of this kind evicted it).
        if (log_n > 24) {
            ctx->cur->va.release(); ctx->cur->vb.release(); ctx->cur->vc.release();
            for (size_t k = 0; k < ctx->plans.size(); ++k)
                if (ctx->plans[k].get() == pl) { ctx->plans.erase(ctx->plans.begin() + (long)k); break; }
        }
    }

    // ---- the same call over the members of a zkhip_multi, the domain sharded (ntt_shard.h).  Every step below is one member's part;
    // the caller (zkhip_api.hip) runs a step on every member before the next on any, because a member fetches what its peers packed
    // in the step before.
    // (the plan's split if this member's plan shards over G members, else -1: the members must agree on it)
    static int ntt_shardable_api(zkhip_ctx* ctx, u32 log_n, u32 G) { const NttPlan<C>* pl = get_plan<C>(ctx, (int)log_n); return shard_ok(pl, G) ? pl->split() : -1; }
    // zkhip_multi_ntt, first step: the member's strip of the input, the outer pass, its blocks packed
    static void shard_ntt_begin(zkhip_ctx* ctx, u32 G, u32 k, u32 log_n, int dir, const uint8_t* data) {
        NttPlan<C>* pl = get_plan<C>(ctx, (int)log_n);
        require(shard_ok(pl, G), ZKHIP_ERR_BAD_ARG, "internal: this transform does not shard");
        const ShardGeom g = ntt_shard_geom(pl->N1, pl->Nb, G);
        Stream s = ctx->stream;
        ctx->ws = s;
        ctx->cur->va.ensure(pl->N * sizeof(Fr));
        shard_state(ctx, g, 1);
        zkhip_ctx::Shard& sh = ctx->shard;
        Fr* a = ptr<Fr>(ctx->cur->va);
        // the strip arrives as the G blocks of its column of blocks, rows back to back: the layout of the staging
        const u64 n = g.range_len();           // (a strip holds as many elements as a range)
        sh.host.resize(n * 32);
        for (u32 r = 0; r < pl->N1; ++r) memcpy(sh.host.data() + (size_t)r * g.W * 32, data + ((size_t)r * pl->Nb + g.strip_origin(k)) * 32, (size_t)g.W * 32);
        dev_h2d(sh.recv.p, sh.host.data(), n * 32, s);
        ZK_LAUNCH((k_mul_const<Fr>), dim3(blocks_for(n, 256)), dim3(256), 0, s, ptr<Fr>(sh.recv), ptr<Fr>(sh.recv), n, pl->k_to_rp);   // canonical -> R'-form
        ZK_LAUNCH((k_ntt_shard_unpack<typename Fr::Params>), dim3(shard_move_blocks(g), 1, G), dim3(256), 0, s, a, ptr<Fr>(sh.recv), shard_move_args(g, k, 0, true, true));
        if (dir == 2)     // coset_fft: x_i * g^i first
            ZK_LAUNCH((k_shard_strip_pow<Fr>), dim3(blocks_for(n, 256)), dim3(256), 0, s, a + g.strip_origin(k), pl->g, pl->N1, ilog2_floor(g.W), pl->Nb, g.strip_origin(k));
        const bool inverse = dir == 1 || dir == 3;
        ntt_cols(ctx, pl, g, k, a, inverse, inverse ? ptr<Fr>(pl->tw_inv) : ptr<Fr>(pl->tw_fwd), 1, 0);
        shard_pack(ctx, g, k, a, 1, 0, true);
    }
    // a member's range (sigma order) to the natural positions of the host vector `out` it holds: permuted (and scaled) on the device
    // into runs of g.rows elements, one run per inner index
    static void range_out(zkhip_ctx* ctx, NttPlan<C>* pl, const ShardGeom& g, u32 k, const Fr* vec, int mode, const Fr& base,
                          const Fr& scale, uint8_t* out) {
        zkhip_ctx::Shard& sh = ctx->shard;
        Stream s = ctx->ws;
        const u64 n = g.range_len();
        sh.out.ensure(n * sizeof(Fr));
        ZK_LAUNCH((k_shard_range_out<Fr>), dim3(blocks_for(n, 256)), dim3(256), 0, s, vec + g.range_origin(k), ptr<Fr>(sh.out), g.rows, pl->Nb, pl->N1, pl->N2, pl->N3,
                  k * g.rows, mode, base, scale);
        sh.host.resize(n * 32);
        dev_d2h(sh.host.data(), sh.out.p, n * 32, s);
        stream_sync(s);
        for (u64 inner = 0; inner < pl->Nb; ++inner)
            memcpy(out + (inner * pl->N1 + (u64)k * g.rows) * 32, sh.host.data() + inner * g.rows * 32, (size_t)g.rows * 32);
    }
    // second step: the peers' blocks, the passes over the member's range, and its part of the output in natural order
    static void shard_ntt_end(zkhip_ctx* ctx, u32 G, u32 k, u32 log_n, int dir, uint8_t* data, zkhip_ctx* const* members) {
        NttPlan<C>* pl = get_plan<C>(ctx, (int)log_n);
        const ShardGeom g = ntt_shard_geom(pl->N1, pl->Nb, G);
        Stream s = ctx->stream;
        ctx->ws = s;
        Fr* a = ptr<Fr>(ctx->cur->va);
        const bool inverse = dir == 1 || dir == 3;
        shard_fetch(ctx, g, k, a, 1, 0, false, members);
        if (pl->log3 > 0) ntt_mid(ctx, pl, g, k, a, inverse, inverse ? ptr<Fr>(pl->tw2_inv) : ptr<Fr>(pl->tw2_fwd), pl->Nb - 1, 1, 0);
        ntt_rows(ctx, pl, g, k, a, inverse, nullptr, 1, 0, 1);
        range_out(ctx, pl, g, k, a, inverse ? 2 : 1, dir == 3 ? pl->g_inv : Fr::one(), pl->n_inv, data);
    }
};

}  // namespace zk
