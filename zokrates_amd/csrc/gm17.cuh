// gm17.cuh — the GM17 proving scheme on the same device machinery (config 5 of BASELINE.json: "second proof system
// behind same Backend trait").
//
// Replaces `<Ark as Backend<T, GM17>>::generate_proof` (/root/reference/zokrates_ark/src/gm17.rs:43-78) from the point
// where the reference hands over to ark — `ProvingKey::deserialize_unchecked` (:60-62) and `GM17::prove` (:64),
// [UPSTREAM] ark-gm17 0.3.0 `create_proof` / `R1CStoSAP::witness_map` — and `NonUniversalBackend<T, GM17>::setup`
// (:19-41, `circuit_specific_setup` -> [UPSTREAM] `generate_parameters` / `R1CStoSAP::instance_map_with_evaluation`).
// Restatement of the algorithm: oracle/gm17.py.
//
// R1CS -> SAP (squares only).  Variables [1, x_1..x_{l-1}, aux_0..aux_{w-1}, e_0..e_{n-1}, f_1..f_{l-1}], M of them;
// rows (D0 = 2n + 2(l-1) + 1, padded to the radix-2 domain D):
//   2k: (A_k+B_k)^2 = 4C_k + e_k     2k+1: (A_k-B_k)^2 = e_k     2n: 1 = 1
//   2n+2i-1: (x_i+1)^2 = 4x_i + f_i  2n+2i: (x_i-1)^2 = f_i
//
// Restructuring that keeps the proof bit-identical (for a fixed key and assignment the three proof points depend on
// d1, d2, r only through rho = r + d1 — d2 cancels — and are unique group elements):
//   A = a_query . ext + rho g_gamma_z                        lane 0   bases [a_query, g_gamma_z, inf]
//   B = b_query . ext + rho h_gamma_z                (G2)    lane 3   bases [b_query, h_gamma_z, inf]
//   C = c_query_1 . ext[l..] + rho g_ab_gamma_z              lane 2   bases [inf x l, c_query_1, g_ab_gamma_z, inf]
//     + rho (c_query_2 . ext)                                lane 1   bases [c_query_2, inf, inf]   (the key carries the 2)
//     + rho^2 g_gamma2_z2                                    host
//     + g_gamma2_z_t . h0,  h0 = (U^2 - W)/Z                 lane 4   bases sigma-permuted like h_query
// with scalars [ext_0..ext_{M-1}, rho, 0]: the four MSMs over the extended assignment share one digit/sort pass, as in
// the Groth16 prover.  ark folds 2 d1 U + d1^2 Z - d2 into the quotient instead; the sums are the same group elements.
//
// The proof-slot driver is the Groth16 prover's (core.cuh, Prover<C>: open_slot, stage_z, start_z_lanes, lanes_after_h, collect,
// run_batch, emit_partial, hand_out_sums, write_proof; the slot's layout is SlotSums<C>), and so is the key loader (PkLoader<C>:
// parse_gm17 maps this scheme's key file to the lanes above, load and check_match serve both schemes).  What this scheme supplies:
// the middle of `enqueue` (SAP rows and the extension on the main stream, the quotient's transforms on the context's NTT stream), the
// host formula for C (`assemble`) and the setup.
#pragma once

namespace zk {

// SAP evaluation vectors and the extension of the assignment from the R1CS row products a = A z, b = B z, c = C z
// (k_matvec), one work-item per R1CS row / per extra row:
//   i < n      : e = (a_i - b_i)^2
//   i == n     : the constant row
//   n < i < n+l: public input x = z[i-n], f = (x-1)^2
// ra/rb/rc/z and sa/sc: R'-form (kernels_ntt.cuh), natural order (the tail [2n+2l-1, D) is zeroed by the caller);
// ext: canonical integers
template <class P>
__global__ void k_sap_rows(const Fe<P>* __restrict__ ra, const Fe<P>* __restrict__ rb, const Fe<P>* __restrict__ rc, const Fe<P>* __restrict__ z,
                           Fe<P>* __restrict__ sa, Fe<P>* __restrict__ sc, Fe<P>* __restrict__ ext, u64 n, u64 l, u64 m) {
    ZK_PRIO_HIGH();
    typedef Fe<P> F;
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + l) return;
    // (sc == nullptr: a key bound to the system carries W's share in its bases — rc is not read, sc not written)
    if (i < n) {
        const F a = ra[i], b = rb[i];
        const F d = fe_sub(a, b);
        const F e = rp_sqr(d);
        sa[2 * i] = fe_add(a, b);
        sa[2 * i + 1] = d;
        if (sc) {
            sc[2 * i] = fe_add(fe_dbl(fe_dbl(rc[i])), e);
            sc[2 * i + 1] = e;
        }
        ext[m + i] = rp_to_plain(e);
    } else if (i == n) {
        sa[2 * n] = rp_one<P>();
        if (sc) sc[2 * n] = rp_one<P>();
    } else {
        const u64 j = i - n;   // 1 <= j < l
        const F x = z[j], one = rp_one<P>();
        const F d = fe_sub(x, one);
        const F f = rp_sqr(d);
        sa[2 * n + 2 * j - 1] = fe_add(x, one);
        sa[2 * n + 2 * j] = d;
        if (sc) {
            sc[2 * n + 2 * j - 1] = fe_add(fe_dbl(fe_dbl(x)), f);
            sc[2 * n + 2 * j] = f;
        }
        ext[m + n - 1 + j] = rp_to_plain(f);
    }
}
// quotient evaluations on the coset, square part: out = a^2 * zinv     (R'-form operand < 2^256, canonical R'-form out); the
// `- c` is subtracted in coefficient form by the last transform (see k_quotient)
template <class P>
__global__ void k_sap_quotient(const Fe<P>* __restrict__ a, Fe<P> zinv, Fe<P>* __restrict__ out, u64 n) {
    ZK_PRIO_HIGH();
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fu<P> aa = fu_sqr_inl(fu_unpack<P>(a[i].v));
    out[i] = rp_canon(fu_mul_inl(aa, fu_unpack<P>(zinv.v)));
}
// setup: the per-variable key scalars (canonical) from u_i(t) = a[i], w_i(t) = c[i]
//   aq = gamma a;  c1 = gamma^2 c + (alpha+beta) gamma a;  c2 = 2 gamma^2 Z a;  vq = gamma c + (alpha+beta) a
template <class F>
__global__ void k_gm17_coeffs(const F* __restrict__ a, const F* __restrict__ c, F gamma, F ab, F two_g2z, F* __restrict__ aq, F* __restrict__ c1,
                              F* __restrict__ c2, F* __restrict__ vq, u64 n) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F v = fe_add(fe_mul(gamma, c[i]), fe_mul(ab, a[i]));
    aq[i] = fe_from_mont(fe_mul(gamma, a[i]));
    c1[i] = fe_from_mont(fe_mul(gamma, v));
    c2[i] = fe_from_mont(fe_mul(two_g2z, a[i]));
    vq[i] = fe_from_mont(v);
}

template <class C>
struct Gm17 {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef PkLoader<C> L;
    typedef Prover<C> P;
    static constexpr int FQB = Fq::BYTES;
    static constexpr int G1B = 2 * FQB, G2B = 4 * FQB;

    // ------------------------------------------------------------ prover
    static Fr add_mod(const Fr& a, const Fr& b) {   // canonical integers
        return fe_from_mont(fe_add(fe_to_mont(a), fe_to_mont(b)));
    }
    // every kernel and copy of one proof, no host synchronisation: the driver of Prover<C>::enqueue with this scheme's middle — the
    // SAP rows and the extension of the assignment on the main stream (they feed the z sort), the quotient's transforms on the
    // context's NTT stream behind them
    static void enqueue(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev,
                        const uint8_t* d1, const uint8_t* r, int check_idx = -1, const PackedZ* zp = nullptr, const WitnessZ* wz = nullptr) {
        L::check_match(pk, cs, 1);
        const u64 m = cs->l + cs->w, n = cs->n, l = cs->l, M = pk->m, D = pk->N;
        Fr dd = fe_from_bytes_canon<Fr>(d1), rr = fe_from_bytes_canon<Fr>(r);
        require(canon_lt_mod(dd) && canon_lt_mod(rr), ZKHIP_ERR_BAD_ARG, "d1 or r not a canonical field element");
        const Fr rho = add_mod(dd, rr);
        const bool bound = P::is_bound(pk, cs);   // (zkhip_pk_bind_r1cs: W's share and the last transform live in the bases)
        NttPlan<C>* pl = P::open_slot(ctx, sl, pk);
        sl.check_idx = check_idx;      // (checked mode, Prover<C>::enqueue_check: the test is on the R1CS rows, not on the SAP's)
        memcpy(sl.r, rho.v, 32);
        memset(sl.s, 0, 32);
        Stream st = ctx->stream;
        P::stage_z(ctx, sl, m, M + 2, z_host, z_dev, check_idx >= 0, false, zp, wz);
        uint8_t* d_scalars = (uint8_t*)sl.scalars.p;
        sl.zmont.ensure(m * 32);
        dev_h2d(d_scalars + M * 32, sl.r, 32, st);
        dev_memset(d_scalars + (M + 1) * 32, 0, 32, st);
        ZK_LAUNCH((k_mul_const<Fr>), dim3(blocks_for(m, 256)), dim3(256), 0, st, (const Fr*)d_scalars, ptr<Fr>(sl.zmont), m, pl->k_to_rp);   // R'-form
        event_record(sl.ev[0], st);

        // ---- SAP rows + the extension of the assignment (K1')
        sl.va.ensure(2 * D * sizeof(Fr));      // the two evaluation vectors back to back: they share every NTT launch
        Fr *sa = ptr<Fr>(sl.va), *sc = sa + D;
        const u64 D0 = 2 * n + 2 * (l - 1) + 1;
        if (D0 < D) {
            dev_memset(sa + D0, 0, (D - D0) * sizeof(Fr), st);
            if (!bound) dev_memset(sc + D0, 0, (D - D0) * sizeof(Fr), st);
        }
        sl.vc.ensure(3 * std::max<u64>(n, 1) * sizeof(Fr));      // the three row-product vectors
        Fr *ra = ptr<Fr>(sl.vc), *rb = ra + n, *rc = rb + n;
        // (checked mode over a bound key: C's rows as well, for the check alone — the SAP rows below still leave W to the bases)
        if (n) P::matvec(ctx, cs, ptr<Fr>(sl.zmont), ra, rb, rc, n, 0, n, (bound && check_idx < 0) ? 2 : 3);
        if (check_idx >= 0) P::enqueue_check(sl, ra, rb, rc, n, st);
        ZK_LAUNCH((k_sap_rows<typename Fr::Params>), dim3(blocks_for(n + l, 256)), dim3(256), 0, st, ra, rb, rc, ptr<Fr>(sl.zmont), sa, bound ? (Fr*)nullptr : sc,
                  (Fr*)d_scalars, n, l, m);
        event_record(sl.ev[1], st);

        // ---- the four MSMs over S = [ext_0..ext_{M-1}, rho, 0] share one digit/sort pass
        const typename P::Lay ly(ctx, pk);
        ly.reserve(sl);
        P::start_z_lanes(ctx, sl, pk, ly);

        // ---- quotient h0 = (U^2 - W)/Z: iNTT + coset NTT of U, pointwise square, coset iNTT minus W's coefficients / Z (sigma order, canonical)
        Stream wn = ctx->serial ? st : ctx_ntt_stream(ctx);
        stream_wait_event(wn, sl.ev[1]);
        ctx->ws = wn;
        event_record(sl.ntt_b, wn);
        // four transforms (ark-gm17's witness_map runs five): W only needs its coefficients, as c in the Groth16 prover.  A bound key:
        // TWO — U^2 / Z(g) in NATURAL order pairs with G' = the coset inverse transform applied to g_gamma2_z_t once (PkLoader::bind),
        // and W's share rides on the c_query_1 lane's bases
        Transforms<C>::ntt_quotient(ctx, pl, sa, 1, sc, bound, [&](const Fr& zinv) {
            ZK_LAUNCH((k_sap_quotient<typename Fr::Params>), dim3(blocks_for(D, 256)), dim3(256), 0, wn, sa, zinv, sa, D);
        });
        ctx->ws = ctx->stream;
        event_record(sl.ntt_e, wn);

        // ---- the lanes over z, and G = MSM(g_gamma2_z_t, h0)   (a bound key: U^2 / Z(g) in natural order against G'); never a lone proof's head start
        P::lanes_after_h(ctx, sl, pk, ly, bound, false, ptr<u32>(sl.va), wn);
    }

    // C = C1 + rho C2 + rho^2 g_gamma2_z2 + G
    static void finish(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, uint8_t* out, zkhip_timings* tm) {
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG, "this proving key is one shard of a multi-GPU key: use zkhip_prove_gm17_partial + zkhip_combine_gm17");
        const typename P::Sums g = P::collect(ctx, sl, pk);
        const auto t_fin = std::chrono::steady_clock::now();
        Fr rho;
        memcpy(rho.v, sl.r, 32);
        if (P::unsatisfied(ctx, sl, typename P::Lay(ctx, pk))) memset(out, 0, P::PROOF_BYTES);      // a refused proof: all zero
        else assemble(pk, g, rho, out);
        P::fill_timings(sl, tm, t_fin);
    }
    static void assemble(const zkhip_pk* pk, const typename P::Sums& g, const Fr& rho, uint8_t* out) {
        const Fr rho2 = fe_from_mont(fe_sqr(fe_to_mont(rho)));
        uint8_t dec[2 * FQB];
        decode_point<FQB, 2>(pk->g_gamma2_z2_canon.data(), dec);
        Aff<Fq> z2;
        memcpy(&z2, dec, sizeof(z2));
        z2 = L::to_mont_point(z2);
        Xyzz<Fq> t1, t2;
        {
            HostThreads th;
            th.run([&] { t1 = xyzz_mul_limbs(g.b1, rho.v, Fr::N); });
            t2 = xyzz_mul_limbs(Xyzz<Fq>::from_affine(z2), rho2.v, Fr::N);
        }
        Xyzz<Fq> gC = xyzz_add(g.l, t1);
        gC = xyzz_add(gC, t2);
        gC = xyzz_add(gC, g.h);
        P::write_proof(g.a.is_inf(), xyzz_to_affine(g.a), g.b2.is_inf(), xyzz_to_affine(g.b2), gC.is_inf(), xyzz_to_affine(gC), out);
    }
    // one rank's share of a proof (as Prover<C>::prove_partial): the five partial sums, canonical records
    static void prove_partial(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev, const uint8_t* rnd,
                              uint8_t* partial_out, zkhip_timings* tm) {
        check_d2(rnd);
        enqueue(ctx, ctx->slots[0], pk, cs, z_host, z_dev, rnd, rnd + 64);
        P::emit_partial(ctx, ctx->slots[0], pk, partial_out, tm);
    }
    // (as Prover<C>::prove_device_sums: the share stays on the device for the RCCL exchange)
    static void prove_device_sums(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const uint8_t* rnd,
                                  const void** d_ws1, size_t* b1, const void** d_ws2, size_t* b2, zkhip_timings* tm) {
        check_d2(rnd);
        enqueue(ctx, ctx->slots[0], pk, cs, z_host, nullptr, rnd, rnd + 64);
        P::hand_out_sums(ctx, ctx->slots[0], pk, d_ws1, b1, d_ws2, b2, tm);
    }
    static void combine(const zkhip_pk* pk, u32 count, const uint8_t* partials, const uint8_t* rnd, uint8_t* out) {
        check_d2(rnd);
        Fr dd = fe_from_bytes_canon<Fr>(rnd), rr = fe_from_bytes_canon<Fr>(rnd + 64);
        require(canon_lt_mod(dd) && canon_lt_mod(rr), ZKHIP_ERR_BAD_ARG, "d1 or r not a canonical field element");
        assemble(pk, P::sum_partials(count, partials), add_mod(dd, rr), out);
    }

    // rnd = d1 | d2 | r (3 x 32 B): d2 is validated and otherwise unused — it cancels out of the proof
    static void check_d2(const uint8_t* rnd) {
        require(canon_lt_mod(fe_from_bytes_canon<Fr>(rnd + 32)), ZKHIP_ERR_BAD_ARG, "d2 not a canonical field element");
    }
    static void prove(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev, const uint8_t* rnd,
                      uint8_t* out, zkhip_timings* tm) {
        check_d2(rnd);
        ctx->unsat.clear();
        enqueue(ctx, ctx->slots[0], pk, cs, z_host, z_dev, rnd, rnd + 64, ctx->checked ? 0 : -1);
        finish(ctx, ctx->slots[0], pk, out, tm);
        P::raise_unsatisfied(ctx, 1, cs);
    }
    // `count` proofs pipelined (Prover<C>::run_batch); rnd: count x 96 B
    static void prove_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, u32 count, const uint8_t* z_host, void* const* z_dev,
                            const uint8_t* rnd, uint8_t* proofs_out, zkhip_timings* tm) {
        const u64 m = cs->l + cs->w;
        P::run_batch(ctx, cs, count, tm,
                     [&](u32 i, ProofSlot& sl) {
                         check_d2(rnd + (size_t)i * 96);
                         enqueue(ctx, sl, pk, cs, z_host ? z_host + (size_t)i * m * 32 : nullptr, z_host ? nullptr : z_dev[i], rnd + (size_t)i * 96,
                                 rnd + (size_t)i * 96 + 64, ctx->checked ? (int)i : -1);
                     },
                     [&](u32 j, ProofSlot& sl, zkhip_timings* one) { finish(ctx, sl, pk, proofs_out + (size_t)j * P::PROOF_BYTES, one); });
    }

    // ------------------------------------------------------------ setup
    // toxic = alpha, beta, gamma, t (4 x 32 B); generators as in zkhip_setup_g16
    static u64 key_bytes(u64 n, u64 l, u64 w) {
        const SapShape sh = sap_shape(n, l, w);
        return (u64)3 * G2B + 2 * G1B + 8 + l * G1B + 8 + sh.M * G1B + 8 + sh.M * G2B + 8 + (sh.M - l) * G1B + 8 + sh.M * G1B + 3 * G1B + G2B + 8 +
               (sh.D + 1) * G1B;
    }
    static void setup(zkhip_ctx* ctx, const zkhip_r1cs* cs, const uint8_t* toxic, const uint8_t* g1b, const uint8_t* g2b, uint8_t* out, u64 cap) {
        typedef Setup<C> S;
        const u64 n = cs->n, l = cs->l, w = cs->w, m = l + w;
        const SapShape sh = sap_shape(n, l, w);
        const u64 M = sh.M, D = sh.D;
        const u64 need = key_bytes(n, l, w);
        require(cap >= need, ZKHIP_ERR_BAD_ARG, "output buffer too small (see zkhip_setup_gm17_size)");
        const Fr alpha = S::read_fr(toxic, false, ""), beta = S::read_fr(toxic + 32, false, "");
        const Fr gamma = S::read_fr(toxic + 64, true, "gamma must be non-zero");
        const Fr t = S::read_fr(toxic + 96, false, "");
        NttPlan<C>* pl = get_plan<C>(ctx, sh.logD);
        const Fr zt = fe_sub(fe_pow_u64(t, D), Fr::one());
        require(!zt.is_zero(), ZKHIP_ERR_BAD_ARG, "t lies in the evaluation domain");
        Stream s = ctx->stream;
        const unsigned T = 256;

        // ---- Lagrange basis at t, then u_i(t), w_i(t) per SAP variable on the host (instance_map_with_evaluation)
        DBuf d_u;
        d_u.ensure(D * sizeof(Fr));
        ZK_LAUNCH((k_lagrange_at<Fr>), dim3(blocks_for(D, T)), dim3(T), 0, s, ptr<Fr>(d_u), t, pl->omega, fe_mul(zt, pl->n_inv), D);
        std::vector<Fr> u(D);
        dev_d2h(u.data(), d_u.p, D * sizeof(Fr), s);
        stream_sync(s);
        std::vector<Fr> av(M, Fr::zero()), cv(M, Fr::zero());
        HostCsr hm;
        hm.fetch(ctx, cs);
        auto val_at = [&](int k, u64 q) { return fe_from_bytes_canon<Fr>(hm.val[k].data() + q * 32); };   // Montgomery form, as resident
        HostThreads ta;
        ta.run([&] {
            for (u64 i = 0; i < n; ++i) {
                const Fr u_add = fe_add(u[2 * i], u[2 * i + 1]), u_sub = fe_sub(u[2 * i], u[2 * i + 1]);
                for (u64 q = hm.rp[0][i]; q < hm.rp[0][i + 1]; ++q) { Fr& x = av[hm.col[0][q]]; x = fe_add(x, fe_mul(u_add, val_at(0, q))); }
                for (u64 q = hm.rp[1][i]; q < hm.rp[1][i + 1]; ++q) { Fr& x = av[hm.col[1][q]]; x = fe_add(x, fe_mul(u_sub, val_at(1, q))); }
            }
            av[0] = fe_add(av[0], u[2 * n]);
            for (u64 i = 1; i < l; ++i) {
                const Fr u1 = u[2 * n + 2 * i - 1], u2 = u[2 * n + 2 * i];
                av[i] = fe_add(av[i], fe_add(u1, u2));
                av[0] = fe_add(av[0], fe_sub(u1, u2));
            }
        });
        for (u64 i = 0; i < n; ++i) {
            const Fr u4 = fe_dbl(fe_dbl(u[2 * i]));
            for (u64 q = hm.rp[2][i]; q < hm.rp[2][i + 1]; ++q) { Fr& x = cv[hm.col[2][q]]; x = fe_add(x, fe_mul(u4, val_at(2, q))); }
            cv[m + i] = fe_add(cv[m + i], fe_add(u[2 * i], u[2 * i + 1]));
        }
        cv[0] = fe_add(cv[0], u[2 * n]);
        for (u64 i = 1; i < l; ++i) {
            const Fr u1 = u[2 * n + 2 * i - 1], u2 = u[2 * n + 2 * i];
            cv[i] = fe_add(cv[i], fe_dbl(fe_dbl(u1)));
            cv[m + n - 1 + i] = fe_add(cv[m + n - 1 + i], fe_add(u1, u2));
        }
        ta.join();

        const Fr ab = fe_add(alpha, beta);
        const Fr gz = fe_mul(gamma, zt), g2z = fe_mul(gamma, gz);
        DBuf d_a, d_c, d_aq, d_c1, d_c2, d_vq, d_t;
        d_a.ensure(M * sizeof(Fr)); d_c.ensure(M * sizeof(Fr));
        d_aq.ensure(M * sizeof(Fr)); d_c1.ensure(M * sizeof(Fr)); d_c2.ensure(M * sizeof(Fr)); d_vq.ensure(M * sizeof(Fr));
        d_t.ensure((D + 1) * sizeof(Fr));
        dev_h2d(d_a.p, av.data(), M * sizeof(Fr), s);
        dev_h2d(d_c.p, cv.data(), M * sizeof(Fr), s);
        ZK_LAUNCH((k_gm17_coeffs<Fr>), dim3(blocks_for(M, T)), dim3(T), 0, s, ptr<Fr>(d_a), ptr<Fr>(d_c), gamma, ab, fe_dbl(g2z), ptr<Fr>(d_aq),
                  ptr<Fr>(d_c1), ptr<Fr>(d_c2), ptr<Fr>(d_vq), M);
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(D + 1, T)), dim3(T), 0, s, ptr<Fr>(d_t), t, g2z, D + 1, 0u, 0u, 0);
        ZK_LAUNCH((k_from_mont<Fr>), dim3(blocks_for(D + 1, T)), dim3(T), 0, s, ptr<Fr>(d_t), ptr<Fr>(d_t), D + 1);
        // single points: G1: alpha, gamma, gamma Z, (alpha+beta) gamma Z, gamma^2 Z^2 ; G2: 1, beta, gamma, gamma Z
        Fr one_c = Fr::zero(); one_c.v[0] = 1;
        Fr singles[9] = {fe_from_mont(alpha), fe_from_mont(gamma), fe_from_mont(gz), fe_from_mont(fe_mul(ab, gz)), fe_from_mont(fe_sqr(gz)),
                         one_c, fe_from_mont(beta), fe_from_mont(gamma), fe_from_mont(gz)};
        DBuf d_single;
        d_single.ensure(sizeof(singles));
        dev_h2d(d_single.p, singles, sizeof(singles), s);
        stream_sync(s);

        DBuf tbl1, tbl2;
        S::template build_table<Fq>(ctx, S::template read_generator<Fq, 2>(g1b, C::g1_gen()), tbl1);
        S::template build_table<Fq2>(ctx, S::template read_generator<Fq2, 4>(g2b, C::g2_gen()), tbl2);
        uint8_t s1[5 * G1B], s2[4 * G2B];
        S::template mul_and_write<Fq, 2>(ctx, tbl1, ptr<Fr>(d_single), 5, s1);
        S::template mul_and_write<Fq2, 4>(ctx, tbl2, ptr<Fr>(d_single) + 5, 4, s2);
        uint8_t* p = out;
        memcpy(p, s2, G2B); p += G2B;                               // vk.h_g2
        memcpy(p, s1, G1B); p += G1B;                               // vk.g_alpha_g1
        memcpy(p, s2 + G2B, G2B); p += G2B;                         // vk.h_beta_g2
        memcpy(p, s1 + G1B, G1B); p += G1B;                         // vk.g_gamma_g1
        memcpy(p, s2 + 2 * G2B, G2B); p += G2B;                     // vk.h_gamma_g2
        p = S::put_len(p, l);
        S::template mul_and_write<Fq, 2>(ctx, tbl1, ptr<Fr>(d_vq), l, p); p += l * G1B;                 // vk.query
        p = S::put_len(p, M);
        S::template mul_and_write<Fq, 2>(ctx, tbl1, ptr<Fr>(d_aq), M, p); p += M * G1B;                 // a_query
        p = S::put_len(p, M);
        S::template mul_and_write<Fq2, 4>(ctx, tbl2, ptr<Fr>(d_aq), M, p); p += M * G2B;                // b_query
        p = S::put_len(p, M - l);
        S::template mul_and_write<Fq, 2>(ctx, tbl1, ptr<Fr>(d_c1) + l, M - l, p); p += (M - l) * G1B;   // c_query_1
        p = S::put_len(p, M);
        S::template mul_and_write<Fq, 2>(ctx, tbl1, ptr<Fr>(d_c2), M, p); p += M * G1B;                 // c_query_2
        memcpy(p, s1 + 2 * G1B, G1B); p += G1B;                     // g_gamma_z
        memcpy(p, s2 + 3 * G2B, G2B); p += G2B;                     // h_gamma_z
        memcpy(p, s1 + 3 * G1B, 2 * G1B); p += 2 * G1B;             // g_ab_gamma_z, g_gamma2_z2
        p = S::put_len(p, D + 1);
        S::template mul_and_write<Fq, 2>(ctx, tbl1, ptr<Fr>(d_t), D + 1, p); p += (D + 1) * G1B;        // g_gamma2_z_t
        require((u64)(p - out) == need, ZKHIP_ERR_DEVICE, "internal: key size mismatch");
    }
};

// ---- the proof queue's share of the two provers (zkhip_queue_*: zkhip_api.hip holds the tickets): ONE proof enqueued exactly as the
// batch calls enqueue theirs (Groth16: lone = false; a checked proof has index 0, it is the only one of its collect), ONE slot
// finished; the scheme is the key's.  rnd = r | s (Groth16) or d1 | d2 | r (GM17).  Everything `enqueue` refuses with ZKHIP_ERR_BAD_ARG
// — a key of another system, a non-canonical blinding scalar, z[0] != 1 — it refuses before its first copy or launch.
template <class C>
struct QueueOps {
    typedef Prover<C> P;
    typedef Gm17<C> G;
    static void check(const zkhip_pk* pk, const zkhip_r1cs* cs) { PkLoader<C>::check_match(pk, cs, pk->scheme); }
    static void enqueue(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev, const PackedZ* zp,
                        const WitnessZ* wz, const uint8_t* rnd, bool checked) {
        const int idx = checked ? 0 : -1;
        if (pk->scheme == 0) {
            P::enqueue(ctx, sl, pk, cs, z_host, z_dev, rnd, rnd + 32, false, idx, zp, wz);
        } else {
            G::check_d2(rnd);
            G::enqueue(ctx, sl, pk, cs, z_host, z_dev, rnd, rnd + 64, idx, zp, wz);
        }
    }
    static void finish(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, uint8_t* out, zkhip_timings* tm) {
        if (pk->scheme == 0) P::finish(ctx, sl, pk, out, tm);
        else G::finish(ctx, sl, pk, out, tm);
    }
};

}  // namespace zk
