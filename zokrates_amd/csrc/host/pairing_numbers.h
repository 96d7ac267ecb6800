// pairing_numbers.h — the per-curve facts of the ate pairing and the few lines of big-integer code that derive its numbers from
// them (host only, start-up only).  Shared by the host verifier (verify.cpp) and by the launcher of the device pairing
// (../pairing.cuh): the loop count, the exponent of the hard part of the final exponentiation and the exponent of the Frobenius
// constant come from p, r and xi here — no table of digits anywhere.
#pragma once
#include <algorithm>
#include <vector>

#include "../field.cuh"

namespace zk {

// ---------------- a little big-integer arithmetic (start-up only) ----------------
typedef std::vector<u32> Big;   // little-endian words, no leading zeros except for the value 0 = {}
inline void big_trim(Big& a) { while (!a.empty() && a.back() == 0) a.pop_back(); }
inline Big big_from(const u32* w, int n) { Big a(w, w + n); big_trim(a); return a; }
inline Big big_small(u64 v) { Big a{(u32)v, (u32)(v >> 32)}; big_trim(a); return a; }
inline int big_cmp(const Big& a, const Big& b) {
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    for (size_t i = a.size(); i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
inline Big big_add(const Big& a, const Big& b) {
    Big r(std::max(a.size(), b.size()) + 1, 0);
    u64 c = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        c += (u64)(i < a.size() ? a[i] : 0) + (i < b.size() ? b[i] : 0);
        r[i] = (u32)c;
        c >>= 32;
    }
    big_trim(r);
    return r;
}
inline Big big_sub(const Big& a, const Big& b) {   // a >= b
    Big r(a.size(), 0);
    u64 bw = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        const u64 t = (u64)a[i] - (i < b.size() ? b[i] : 0) - bw;
        r[i] = (u32)t;
        bw = (t >> 63) & 1;
    }
    big_trim(r);
    return r;
}
inline Big big_mul(const Big& a, const Big& b) {
    Big r(a.size() + b.size() + 1, 0);
    for (size_t i = 0; i < a.size(); ++i) {
        u64 c = 0;
        for (size_t j = 0; j < b.size() || c; ++j) {
            c += (u64)r[i + j] + (j < b.size() ? (u64)a[i] * b[j] : 0);
            r[i + j] = (u32)c;
            c >>= 32;
        }
    }
    big_trim(r);
    return r;
}
inline int big_bits(const Big& a) { return a.empty() ? 0 : 32 * (int)(a.size() - 1) + (32 - __builtin_clz(a.back())); }
inline bool big_bit(const Big& a, int i) { return (size_t)(i >> 5) < a.size() && ((a[i >> 5] >> (i & 31)) & 1); }
// floor(a / b) and the remainder, shift-and-subtract (a few thousand word operations: start-up only)
inline Big big_divmod(const Big& a, const Big& b, Big* rem) {
    Big q((a.size() ? a.size() : 1), 0), r;
    for (int i = big_bits(a) - 1; i >= 0; --i) {
        u32 carry = big_bit(a, i);                  // r = 2 r + bit i of a
        for (size_t k = 0; k < r.size(); ++k) { const u32 nc = r[k] >> 31; r[k] = (r[k] << 1) | carry; carry = nc; }
        if (carry) r.push_back(carry);
        if (big_cmp(r, b) >= 0) { r = big_sub(r, b); q[i >> 5] |= 1u << (i & 31); }
    }
    big_trim(q);
    if (rem) *rem = r;
    return q;
}

// ---------------- per-curve facts ----------------
template <class P> struct PairingCfg;      // XI0: xi = XI0 + u; LOOP: the ate loop count t - 1 (0: p - r, the BN case)
template <> struct PairingCfg<Bn254Fq> {     // y^2 = x^3 + 3; twist y^2 = x^3 + 3 / xi (type D), xi = 9 + u
    typedef Bn254Fr Fr;
    static constexpr u32 XI0 = 9, B = 3;
    static constexpr bool D_TWIST = true;
    static constexpr u64 LOOP = 0;
};
template <> struct PairingCfg<Bls381Fq> {    // y^2 = x^3 + 4; twist y^2 = x^3 + 4 xi (type M), xi = 1 + u; |x| = 0xd201000000010000
    typedef Bls381Fr Fr;
    static constexpr u32 XI0 = 1, B = 4;
    static constexpr bool D_TWIST = false;
    static constexpr u64 LOOP = 0xd201000000010000ull;
};
template <> struct PairingCfg<Bls377Fq> {    // y^2 = x^3 + 1; twist y^2 = x^3 + 1 / xi (type D), xi = u (u^2 = -5); x = 0x8508c00000000001
    typedef Bls377Fr Fr;
    static constexpr u32 XI0 = 0, B = 1;
    static constexpr bool D_TWIST = true;
    static constexpr u64 LOOP = 0x8508c00000000001ull;
};

template <class P> Big modulus_of() { u32 w[P::N]; for (int i = 0; i < P::N; ++i) w[i] = P::mod(i); return big_from(w, P::N); }

// p, r, the loop count t - 1, the hard exponent (p^4 - p^2 + 1) / r and the Frobenius exponent (p - 1) / 6.
// Returns nullptr, or what is wrong with the curve's numbers (never, for the three curves above)
struct PairingNumbers { Big p, r, loop, hard, frob; };
template <class P>
const char* pairing_numbers(PairingNumbers& n) {
    typedef PairingCfg<P> Cfg;
    n.p = modulus_of<P>();
    n.r = modulus_of<typename Cfg::Fr>();
    n.loop = Cfg::LOOP ? big_small(Cfg::LOOP) : big_sub(n.p, n.r);
    const Big p2 = big_mul(n.p, n.p), p4 = big_mul(p2, p2);
    Big rem;
    n.hard = big_divmod(big_add(big_sub(p4, p2), big_small(1)), n.r, &rem);
    if (!rem.empty()) return "pairing: r does not divide p^4 - p^2 + 1";
    n.frob = big_divmod(big_sub(n.p, big_small(1)), big_small(6), &rem);
    if (!rem.empty()) return "pairing: p != 1 mod 6";
    return nullptr;
}

}  // namespace zk
