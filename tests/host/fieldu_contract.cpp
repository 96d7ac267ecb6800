// TEST ONLY: a thin driver over the unsaturated field of fieldu.cuh for tests/test_fieldu_contract.py.
// stdin: one case per line, "<field> <op> <hex word> ...": the operands' raw limbs (or packed words) back to back; they go
// into Fu<P> / Fu2<P> objects exactly as given, never through fu_from_fe.  stdout: one line per case with the raw result
// (limbs, packed words or a truth value).  After the last case: "count <field> <op> <n>" per pair that ran.
// What a result must satisfy is decided by the Python side alone (big integers); nothing is judged here.  A column that
// leaves 64 bits or a lazily subtracted top limb above its bias aborts the program (-DZK_CHECK_OVERFLOW).
#undef _FORTIFY_SOURCE    // the fibre emulator switches stacks with _setjmp / _longjmp (tests/_emu/build_emu.sh builds without it too)
#define ZK_EMU 1          // kernels_ntt.cuh on the host: rp_canon and the passes' product fu_mul_ntt as the kernels have them
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include <iostream>
#include "ec.cuh"
#include "kernels_ntt.cuh"
using namespace zk;

typedef std::vector<u32> Words;
template <class P> static Fu<P> take(const Words& w, size_t& at) {
    Fu<P> r;
    if (at + Fu<P>::N > w.size()) { fprintf(stderr, "driver: too few operand words\n"); exit(3); }
    for (int i = 0; i < Fu<P>::N; ++i) r.v[i] = w[at++];
    return r;
}
template <class P> static Fu2<P> take2(const Words& w, size_t& at) { Fu<P> a = take<P>(w, at), b = take<P>(w, at); return {a, b}; }
template <class P> static void put(Words& o, const Fu<P>& a) { for (int i = 0; i < Fu<P>::N; ++i) o.push_back(a.v[i]); }
template <class P> static void put(Words& o, const Fu2<P>& a) { put(o, a.c0); put(o, a.c1); }

// the extension's forms only exist over a base field (P::BETA)
template <class P, bool FQ> struct Ext { static bool run(const std::string&, const Words&, size_t&, Words&) { return false; } };
template <class P> struct Ext<P, true> {
    static bool run(const std::string& op, const Words& w, size_t& at, Words& o) {
        typedef Fu2<P> U2;
        if (op == "ec_mul2x") { U2 a = take2<P>(w, at), b = take2<P>(w, at); put(o, ec_mul(a, b)); }
        else if (op == "ec_sqr2x") { U2 a = take2<P>(w, at); put(o, ec_sqr(a)); }
        else if (op == "fu2_mul_loose") { U2 a = take2<P>(w, at), b = take2<P>(w, at); put(o, fu2_mul_inl<P, true>(a, b)); }
        else if (op == "fu2_sqr_loose") { U2 a = take2<P>(w, at); put(o, fu2_sqr_inl<P, true>(a)); }
        else if (op == "fu2_mulsub_loose") { U2 a = take2<P>(w, at), b = take2<P>(w, at), c = take2<P>(w, at), d = take2<P>(w, at); put(o, fu2_mulsub_inl<P, true>(a, b, c, d)); }
        else if (op == "fu2_mul_kara") { U2 a = take2<P>(w, at), b = take2<P>(w, at); put(o, fu2_mul_kara(a, b)); }
        else if (op == "ec_inv2x") { U2 a = take2<P>(w, at); put(o, ec_inv(a)); }
        else return false;
        return true;
    }
};

template <class P, bool FQ> static bool run(const std::string& op, const Words& w, Words& o) {
    typedef Fu<P> U;
    size_t at = 0;
    if (op == "info") {      // B N W LOOSE_OK
        o = {(u32)U::B, (u32)U::N, (u32)P::N, (u32)(ZK_LOOSE_M && UConst<P>::LOOSE_OK)};
    } else if (op == "fe_add") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fe_add(a, b)); }
    else if (op == "fe_dbl") { U a = take<P>(w, at); put(o, fe_dbl(a)); }
    else if (op == "fe_sub_k2") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fe_sub_k<2>(a, b)); }
    else if (op == "fe_sub_k4") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fe_sub_k<4>(a, b)); }
    else if (op == "fe_sub_k8") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fe_sub_k<8>(a, b)); }
    else if (op == "fe_sub_k16") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fe_sub_k<16>(a, b)); }
    else if (op == "fe_neg") { U a = take<P>(w, at); put(o, fe_neg(a)); }
    else if (op == "fe_cneg") { U a = take<P>(w, at); put(o, fe_cneg(a, true)); put(o, fe_cneg(a, false)); }
    else if (op == "fe_relax") { U a = take<P>(w, at); put(o, fe_relax(a)); }
    else if (op == "fe_is_zero_modp") { U a = take<P>(w, at); o.push_back(fe_is_zero_modp(a) ? 1u : 0u); }
    else if (op == "rp_canon") { U a = take<P>(w, at); Fe<P> r = rp_canon(a); for (int i = 0; i < P::N; ++i) o.push_back(r.v[i]); }
    else if (op == "fu_pack") { U a = take<P>(w, at); u32 k[P::N]; fu_pack(a, k); for (int i = 0; i < P::N; ++i) o.push_back(k[i]); }
    else if (op == "fu_unpack") {      // packed words -> limbs, and packed again
        if (w.size() != (size_t)P::N) { fprintf(stderr, "driver: fu_unpack wants the packed words\n"); exit(3); }
        at = w.size();
        U a = fu_unpack<P>(w.data());
        put(o, a);
        u32 k[P::N]; fu_pack(a, k); for (int i = 0; i < P::N; ++i) o.push_back(k[i]);
    }
    else if (op == "fu_mul_inl") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fu_mul_inl(a, b)); }
    else if (op == "fu_sqr_inl") { U a = take<P>(w, at); put(o, fu_sqr_inl(a)); }
    else if (op == "fu_mul2_inl") { U a = take<P>(w, at), b = take<P>(w, at), c = take<P>(w, at), d = take<P>(w, at); put(o, fu_mul2_inl<P>(a, b, c, d)); }
    else if (op == "fu_mul4_inl") {
        U a = take<P>(w, at), b = take<P>(w, at), c = take<P>(w, at), d = take<P>(w, at), e = take<P>(w, at), f = take<P>(w, at), g = take<P>(w, at), h = take<P>(w, at);
        put(o, fu_mul4_inl<P>(a, b, c, d, e, f, g, h));
    }
    else if (op == "fu_mul_loose") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fu_mul_loose(a, b)); }
    else if (op == "fu_sqr_loose") { U a = take<P>(w, at); put(o, fu_sqr_loose(a)); }
    else if (op == "fu_x3_numerator") { U a = take<P>(w, at), b = take<P>(w, at), c = take<P>(w, at); put(o, fu_x3_numerator(a, b, c)); }
    // the lazy forms, each inside the one product its comment allows
    else if (op == "mul_neg_lazy") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fu_mul_inl(fe_neg_lazy(a), b)); }
    else if (op == "mul_loose_neg_lazy") { U a = take<P>(w, at), b = take<P>(w, at); put(o, fu_mul_loose(fe_neg_lazy(a), b)); }
    else if (op == "mul2_neg_lazy") { U a = take<P>(w, at), b = take<P>(w, at), c = take<P>(w, at), d = take<P>(w, at); put(o, fu_mul2_inl<P>(a, b, c, fe_neg_lazy(d))); }
    else if (op == "mul2_loose_neg_lazy") { U a = take<P>(w, at), b = take<P>(w, at), c = take<P>(w, at), d = take<P>(w, at); put(o, fu_mul2_inl<P, true>(a, b, c, fe_neg_lazy(d))); }
    else if (op == "mul_cneg_for_mul") { U y = take<P>(w, at), b = take<P>(w, at); put(o, fu_mul_inl(b, fe_cneg_for_mul(y, true))); put(o, fu_mul_inl(b, fe_cneg_for_mul(y, false))); }
    else if (op == "mul2_cneg_for_mul") { U a = take<P>(w, at), b = take<P>(w, at), c = take<P>(w, at), y = take<P>(w, at); put(o, fu_mul2_inl<P>(a, b, c, fe_cneg_for_mul(y, true))); }
    else if (op == "ntt_sub_lazy2") { U a = take<P>(w, at), b = take<P>(w, at), t = take<P>(w, at); put(o, fu_mul_ntt<P>(fe_sub_k_lazy<2>(a, b), t)); }
    else if (op == "ntt_sub_lazy4") { U a = take<P>(w, at), b = take<P>(w, at), t = take<P>(w, at); put(o, fu_mul_ntt<P>(fe_sub_k_lazy<4>(a, b), t)); }
    else if (op == "ntt_sub_lazy8") { U a = take<P>(w, at), b = take<P>(w, at), t = take<P>(w, at); put(o, fu_mul_ntt<P>(fe_sub_k_lazy<8>(a, b), t)); }
    else if (op == "ntt_add_lazy") { U a = take<P>(w, at), b = take<P>(w, at), t = take<P>(w, at); put(o, fu_mul_ntt<P>(fe_add_lazy(a, b), t)); }
    else if (op == "ntt_first_round" || op == "lds_ntt_dif4" || op == "lds_ntt_last4") {
        if constexpr (U::N <= (int)NTT_PLAN_STRIDE) {      // (a plan entry holds 12 limbs: the nine-limb fields the passes compute in)
            constexpr int logn = 4, n = 16, q = 4, PL = 32;
            const u32 plen = ntt_plan_len(logn);
            alignas(16) static u32 plan[16 * NTT_PLAN_STRIDE];
            static u32 lds[U::N * PL];
            memset(plan, 0, sizeof plan);
            memset(lds, 0, sizeof lds);
            if (op == "ntt_first_round") {
                // the kernels' own radix-4 butterfly on four elements and four factors: a 16-point sub-transform's first round at
                // position 1, a plain array as its LDS planes and a plan that holds the factors where the butterfly looks for them
                U a = take<P>(w, at), bq = take<P>(w, at), c = take<P>(w, at), d = take<P>(w, at);
                const U f1 = take<P>(w, at), f2 = take<P>(w, at), f3 = take<P>(w, at), f4 = take<P>(w, at);     // w^pos, w^2pos, w^3pos, w4
                constexpr int pos = 1;
                const U* fs[4] = {&f1, &f2, &f3, &f4};
                const u32 where[4] = {(u32)pos, (u32)(q + pos), (u32)(2 * q + pos), plen - 1};
                for (int k = 0; k < 4; ++k) for (int l = 0; l < U::N; ++l) plan[where[k] * NTT_PLAN_STRIDE + l] = fs[k]->v[l];
                ntt_first_round<P>(lds, PL, 0, logn, pos, a, bq, c, d, plan, plen);
                for (int k = 0; k < 4; ++k) put(o, lds_get_u<P>(lds, PL, ntt_slot(pos + k * q)));
            } else if (op == "lds_ntt_last4") {
                // the last, untwiddled round alone (a 4-point sub-transform: its plan is w4), so that its carried differences meet
                // inputs at the top of their range directly
                for (int e = 0; e < 4; ++e) { const U x = take<P>(w, at); lds_put_u<P>(lds, PL, ntt_slot(e), x); }
                const U f = take<P>(w, at);
                for (int l = 0; l < U::N; ++l) plan[l] = f.v[l];
                emu::launch(dim3(1), dim3(1), 0, [&] { lds_ntt_dif4<P>(lds, PL, ntt_seq_stride(4), 2, 1, plan, 1, false); });
                for (int e = 0; e < 4; ++e) put(o, lds_get_u<P>(lds, PL, ntt_slot(e)));
            } else {
                // the whole LDS-resident 16-point sub-transform (a twiddled round and the last, untwiddled one) as a workgroup of four
                // work-items on the fibre emulator: 16 elements, then the 13 entries of the plan; the 16 slots come back as they are left
                for (int e = 0; e < n; ++e) { const U x = take<P>(w, at); lds_put_u<P>(lds, PL, ntt_slot(e), x); }
                for (u32 k = 0; k < plen; ++k) { const U f = take<P>(w, at); for (int l = 0; l < U::N; ++l) plan[k * NTT_PLAN_STRIDE + l] = f.v[l]; }
                emu::launch(dim3(1), dim3(4), 0, [&] { lds_ntt_dif4<P>(lds, PL, ntt_seq_stride(n), logn, 1, plan, plen, false); });
                for (int e = 0; e < n; ++e) put(o, lds_get_u<P>(lds, PL, ntt_slot(e)));
            }
        } else return false;
    }
    else if (op == "ec_inv") { U a = take<P>(w, at); put(o, ec_inv(a)); }
    else if (!Ext<P, FQ>::run(op, w, at, o)) return false;
    if (at != w.size()) { fprintf(stderr, "driver: %s: %zu operand words left over\n", op.c_str(), w.size() - at); exit(3); }
    return true;
}

int main() {
    std::map<std::string, unsigned long> count;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string field, op, tok;
        in >> field >> op;
        Words w, o;
        while (in >> tok) w.push_back((u32)strtoul(tok.c_str(), nullptr, 16));
        bool ok = false;
        if (field == "Bn254Fq") ok = run<Bn254Fq, true>(op, w, o);
        else if (field == "Bls381Fq") ok = run<Bls381Fq, true>(op, w, o);
        else if (field == "Bls377Fq") ok = run<Bls377Fq, true>(op, w, o);
        else if (field == "Bn254Fr") ok = run<Bn254Fr, false>(op, w, o);
        else if (field == "Bls381Fr") ok = run<Bls381Fr, false>(op, w, o);
        else if (field == "Bls377Fr") ok = run<Bls377Fr, false>(op, w, o);
        if (!ok) { fprintf(stderr, "driver: unknown field / op: %s %s\n", field.c_str(), op.c_str()); return 3; }
        ++count[field + " " + op];
        std::string out;
        char buf[16];
        for (size_t i = 0; i < o.size(); ++i) { snprintf(buf, sizeof buf, i ? " %x" : "%x", o[i]); out += buf; }
        out += "\n";
        fputs(out.c_str(), stdout);
    }
    for (const auto& kv : count) printf("count %s %lu\n", kv.first.c_str(), kv.second);
    return 0;
}
