// pairing.cuh — the pairing check on the device: Fq12 tower arithmetic, Miller loop and final exponentiation over the unsaturated
// limbs of fieldu.cuh, one verdict per item (product code; instantiated from the curve_*.hip units).
//
// What it computes is what csrc/host/verify.cpp computes on one host thread — prod_k e(P_k, Q_k) == 1 by the plain ate loop on
// the twist (loop count t - 1, no Frobenius end-steps), Fq12 = Fq2[w] / (w^6 - xi) as six Fq2 coefficients, the easy part of the
// final exponentiation by conj6, inverse and Frobenius^2, the hard part by square-and-multiply over (p^4 - p^2 + 1) / r — for many
// items at once.  Only the verdict is specified: the Miller value differs from the host's by factors of Fq2 (the host's affine
// steps invert in Fq2 at every step; here the steps are homogeneous projective, and a line is scaled by its denominator, which
// lies in a proper subfield and dies in the easy part).
//
// Work decomposition.  One Fq12 is 108 (BN254) or 168 (BLS) limbs; a lane that owned a whole item would keep three of them live
// and spill.  So an item belongs to a GROUP of PAIR_LANES = 8 lanes: lane k < 6 owns coefficient k of every Fq12 value of its
// item, lane j < pairs_per_item also owns pair j (its running point T on the twist, in registers), and the values themselves
// live in LDS (PairLds: four Fq12 "registers" and one line per item).  A product is then six schoolbook Fq2 products per lane
// (three for a line) whose operands are read from LDS — all lanes of a group read a_i at the same address (a broadcast) — one
// multiplication by xi on small constants, and one store.  A wavefront carries PAIR_ITEMS = 8 items and a workgroup is one
// wavefront, so the barriers between a product's reads and its store cost a wave nothing.  Per lane the kernel holds T, the
// three values of a line and one product's columns: no Fq12 value is ever in registers.
//
// Bounds (fieldu.cuh's terms).  Every Fq12 coefficient in LDS, every coordinate of T and every line value is TIGHT with both
// components < 3p (each ends in fe_relax); Fq2 products take operands < 8p and return < 2p; the bounds of every function are
// written beside it.
#pragma once
#include <type_traits>

#include "ec.cuh"
#include "host/pairing_numbers.h"

namespace zk {

#ifndef ZK_EMU
#define ZK_NOUNROLL _Pragma("unroll 1")
#else
#define ZK_NOUNROLL
#endif

static constexpr int PAIR_LANES = 8;                 // lanes of one item's group
static constexpr int PAIR_ITEMS = 64 / PAIR_LANES;   // g: items one wavefront (= one workgroup) carries
static constexpr u32 PAIR_MAX_PAIRS = PAIR_LANES;    // pairs of one item: one lane each
static constexpr int TOWER_OPS = 6;                  // zkhip_tower_op: 0 mul, 1 sqr, 2 sparse mul, 3 inverse, 4 Frobenius, 5 conj6

// point status, written by k_pair_admit: what the pairing kernel and the host do with a point
enum : uint8_t { PT_GOOD = 0, PT_INF = 1, PT_REFUSED = 2, PT_NONCANON = 3 };

// the numbers a curve's kernels take by value, derived on the host from p, r and xi (PairingDev::consts)
template <class P>
struct PairConsts {
    Fu2<P> gamma[6];      // gamma[i] = xi^(i (p - 1) / 6): (c w^i)^p = conj(c) gamma[i] w^i.  Canonical: < p
    Fu2<P> b3;            // three times the twist's coefficient b' (b / xi on a type D twist, b xi on a type M one).  < 2p
    u32 loop[4];          // the ate loop count t - 1
    int loop_bits;
    u32 hard[40];         // (p^4 - p^2 + 1) / r
    int hard_bits;
};
template <class P>
struct AdmitConsts {
    Fe<P> b1;             // the curve's b, Montgomery form
    Fe2<P> b2;            // the twist's b'
    u32 r[8];             // the group order
};

// one item's exchange area in LDS
template <class P>
struct PairLds {
    Fu2<P> reg[4][6];     // four Fq12 values, coefficient k written by lane k only
    Fu2<P> line[3];       // the values of the line being multiplied in, in the order of their positions
    u32 skip;             // that line belongs to a pair with a point at infinity: it contributes 1
    u32 bad[PAIR_LANES];  // pair j holds a point that was refused
    u32 vote[PAIR_LANES]; // coefficient k of the result is the coefficient of 1
};

// K a, K in {0, 1, 5, 9} (the small constants of the three xi and of BETA).  a: TIGHT, < 3p.  Result TIGHT, < 3p
template <u32 K, class P>
ZK_HD Fu<P> fu_times_small(const Fu<P>& a) {
    static_assert(K == 0 || K == 1 || K == 5 || K == 9, "fu_times_small: 0, 1, 5 or 9");
    if constexpr (K == 0) return Fu<P>::zero();
    else if constexpr (K == 1) return a;
    else {
        Fu<P> t = fe_dbl(fe_dbl(a));                 // < 12p
        if constexpr (K == 9) t = fe_dbl(t);         // < 24p
        return fe_relax(fe_add(t, a));               // < 27p before, < 3p after
    }
}
// xi a = (XI0 a0 - BETA a1) + (a0 + XI0 a1) u.  a: components TIGHT, < 3p.  Result: TIGHT, c0 < 7p, c1 < 6p (a subtrahend for sub<8>)
template <class P>
ZK_HD Fu2<P> f2_mul_xi(const Fu2<P>& a) {
    constexpr u32 X = PairingCfg<P>::XI0;
    const Fu<P> ba1 = fu_times_small<P::BETA>(a.c1);                 // < 3p: top limb far below (4p)_top - 2
    if constexpr (X == 0) return {fe_sub_k<4>(Fu<P>::zero(), ba1), a.c0};
    else return {fe_sub_k<4>(fu_times_small<X>(a.c0), ba1), fe_add(a.c0, fu_times_small<X>(a.c1))};
}
// a s for s in Fq.  a's components and s TIGHT, < 8p.  Result < 2p
template <class P>
ZK_HD Fu2<P> f2_scale(const Fu2<P>& a, const Fu<P>& s) { return {fu_mul_inl(a.c0, s), fu_mul_inl(a.c1, s)}; }
// the position (power of w) of the t-th value of a line: 1, w, w^3 on a type D twist; 1, w^2, w^3 on a type M one
template <class P>
ZK_HD int line_pos(int t) { return t == 0 ? 0 : t == 1 ? (PairingCfg<P>::D_TWIST ? 1 : 2) : 3; }

// Coefficient k (0 <= k < 6) of a b, where a is a whole Fq12 (six coefficients) and b is a whole Fq12 (NT = 6) or a line (NT = 3
// values at line_pos).  Term a_i b_j lands on w^(i + j); those with i + j >= 6 are summed apart and multiplied by xi once.
// Operands: components TIGHT, < 3p.  lo <= 6 products < 12p, hi <= 5 products < 10p -> relaxed < 3p -> xi: < 7p; sum < 19p.
// Result: TIGHT, < 3p.  One site of the Fq2 product per instantiation (the loop is not unrolled)
template <class P, int NT>
ZK_HD Fu2<P> f12_coef(const Fu2<P>* a, const Fu2<P>* b, int k) {
    Fu2<P> lo = Fu2<P>::zero(), hi = Fu2<P>::zero();
    ZK_NOUNROLL for (int t = 0; t < NT; ++t) {
        const int jb = NT == 6 ? t : line_pos<P>(t);
        int i = k - jb;
        const bool wrap = i < 0;
        if (wrap) i += 6;
        const Fu2<P> x = a[i], y = b[t];
        const Fu2<P> s = fe_add(fe_select(wrap, hi, lo), fu2_mul_inl<P>(x, y));
        lo = fe_select(wrap, lo, s);
        hi = fe_select(wrap, s, hi);
    }
    return fe_relax(fe_add(lo, f2_mul_xi<P>(fe_relax(hi))));
}

// ---- Fq12 on a group: every lane of the workgroup calls these in the same order (they hold barriers); k = the lane within its
// group, lanes 6 and 7 only keep the barriers.  On entry every earlier store is behind a barrier; the same holds on return.
// reg[d] = reg[a] reg[b]; d may be a or b
template <class P>
ZK_HD void f12_mul(PairLds<P>* L, int d, int a, int b, int k) {
    Fu2<P> r = Fu2<P>::zero();
    if (k < 6) r = f12_coef<P, 6>(L->reg[a], L->reg[b], k);
    __syncthreads();
    if (k < 6) L->reg[d][k] = r;
    __syncthreads();
}
// reg[d] = reg[a] (line), line = L->line; keep: leave reg[d] as it is (the line of a pair at infinity)
template <class P>
ZK_HD void f12_mul_line(PairLds<P>* L, int d, int a, int k, bool keep) {
    Fu2<P> r = Fu2<P>::zero();
    if (k < 6) r = f12_coef<P, 3>(L->reg[a], L->line, k);
    __syncthreads();
    if (k < 6 && !keep) L->reg[d][k] = r;
    __syncthreads();
}
// reg[d] = reg[a]^(p^6): w -> -w.  < 4p relaxed to < 3p
template <class P>
ZK_HD void f12_conj6(PairLds<P>* L, int d, int a, int k) {
    if (k < 6) {
        const Fu2<P> v = L->reg[a][k];
        L->reg[d][k] = (k & 1) ? fe_relax(fe_sub_k<4>(Fu2<P>::zero(), v)) : v;
    }
    __syncthreads();
}
// reg[d] = reg[a]^p: coefficient k is conj(c_k) gamma[k].  The conjugate's c1 is 4p - c1 < 4p; the product is < 2p
template <class P>
ZK_HD void f12_frobenius(PairLds<P>* L, int d, int a, int k, const PairConsts<P>& c) {
    if (k < 6) {
        Fu2<P> v = L->reg[a][k];
        v.c1 = fe_sub_k<4>(Fu<P>::zero(), v.c1);
        L->reg[d][k] = fu2_mul_inl<P>(v, c.gamma[k]);
    }
    __syncthreads();
}
// reg[d] = 1
template <class P>
ZK_HD void f12_set_one(PairLds<P>* L, int d, int k) {
    if (k < 6) L->reg[d][k] = k == 0 ? Fu2<P>::one() : Fu2<P>::zero();
    __syncthreads();
}
// reg[d] = 1 / n for an n in Fq6 = Fq2[v] / (v^3 - xi), v = w^2 (reg[a] with its odd coefficients zero).  Every lane computes the
// three cofactors from the same three coefficients; lane 0, 2, 4 keeps its own.  d != a.  (0 -> 0)
// t0 = a0^2 - xi a1 a2 < 10p, t1 = xi a2^2 - a0 a1 < 9p, t2 = a1^2 - a0 a2 < 4p, each relaxed to < 3p; the norm
// a0 t0 + xi (a2 t1 + a1 t2) < 9p is relaxed before ec_inv (operands < 8p)
template <class P>
ZK_HD void f12_inv_fq6(PairLds<P>* L, int d, int a, int k) {
    if (k < 6) {
        const Fu2<P> a0 = L->reg[a][0], a1 = L->reg[a][2], a2 = L->reg[a][4];
        const Fu2<P> t0 = fe_relax(fe_sub_k<8>(ec_sqr(a0), f2_mul_xi<P>(ec_mul(a1, a2))));
        const Fu2<P> t1 = fe_relax(fe_sub_k<2>(f2_mul_xi<P>(ec_sqr(a2)), ec_mul(a0, a1)));
        const Fu2<P> t2 = fe_relax(fe_sub_k<2>(ec_sqr(a1), ec_mul(a0, a2)));
        const Fu2<P> s = fe_relax(fe_add(ec_mul(a2, t1), ec_mul(a1, t2)));
        const Fu2<P> n = fe_relax(fe_add(ec_mul(a0, t0), f2_mul_xi<P>(s)));
        const Fu2<P> di = ec_inv(n);
        const Fu2<P> mine = fe_select(k == 0, t0, fe_select(k == 2, t1, t2));
        const Fu2<P> v = ec_mul(mine, di);
        L->reg[d][k] = (k & 1) ? Fu2<P>::zero() : v;
    }
    __syncthreads();
}
// reg[d] = 1 / reg[a] = conj6(a) / (a conj6(a)); the norm lies in Fq6.  tc, tn, d, a: four different registers but tn may be d
template <class P>
ZK_HD void f12_inverse(PairLds<P>* L, int d, int a, int tc, int tn, int tni, int k) {
    f12_conj6(L, tc, a, k);
    f12_mul(L, tn, a, tc, k);
    f12_inv_fq6(L, tni, tn, k);
    f12_mul(L, d, tc, tni, k);
}

// ---- the steps of the Miller loop on the twist y^2 = x^3 + b', T = (X : Y : Z) homogeneous (x = X / Z, y = Y / Z), coordinates
// TIGHT < 3p.  A line through T with slope n / m, evaluated at the image of P = (xP, yP), is scaled by m (in Fq2):
//     l = m yP  -  n xP w  +  (n xT - m yT) w^3          (type D; type M: the same three values at w^3, w^2, 1)
// l0, l1, l2: the three values in the order of line_pos.  yP, nxP = -xP: TIGHT < 2p.
// doubling: n / m = 3 X^2 / (2 Y Z), and with X^3 = Y^2 Z - b' Z^3 the constant term is Y^2 - 3 b' Z^2:
//     X3 = 2 X Y (Y^2 - 9 b' Z^2),  Y3 = (Y^2 + 9 b' Z^2)^2 - 12 (3 b' Z^2)^2,  Z3 = 8 Y^3 Z
template <class P>
ZK_HD void pair_dbl_step(Fu2<P>& X, Fu2<P>& Y, Fu2<P>& Z, const Fu<P>& yP, const Fu<P>& nxP, const Fu2<P>& b3, Fu2<P>& l0, Fu2<P>& l1, Fu2<P>& l2) {
    typedef Fu2<P> F;
    const F A = ec_sqr(X), B = ec_sqr(Y), C = ec_sqr(Z);            // < 2p
    const F D = ec_mul(b3, C);                                      // 3 b' Z^2 < 2p
    const F H = fe_dbl(ec_mul(Y, Z));                               // 2 Y Z < 4p
    const F ly = f2_scale(H, yP);                                   // < 2p
    const F lx = f2_scale(fe_add(fe_dbl(A), A), nxP);               // 3 X^2 < 6p
    const F lc = fe_relax(fe_sub_k<2>(B, D));                       // < 4p -> < 3p
    const F D3 = fe_add(fe_dbl(D), D);                              // 9 b' Z^2 < 6p
    const F XY = ec_mul(X, Y);
    X = fe_relax(fe_dbl(ec_mul(XY, fe_relax(fe_sub_k<8>(B, D3)))));   // B + 8p - D3 < 10p -> < 3p; 2 (product) < 4p -> < 3p
    const F S2 = ec_sqr(fe_relax(fe_add(B, D3)));                   // < 8p -> < 3p (a square takes < 6p)
    const F D2 = ec_sqr(D);
    const F D12 = fe_relax(fe_dbl(fe_dbl(fe_add(fe_dbl(D2), D2)))); // 12 D^2 < 24p -> < 3p
    Y = fe_relax(fe_sub_k<4>(S2, D12));                             // < 6p -> < 3p
    Z = fe_relax(fe_dbl(fe_dbl(ec_mul(B, H))));                     // 4 B H < 8p -> < 3p
    l0 = PairingCfg<P>::D_TWIST ? ly : lc;
    l1 = lx;
    l2 = PairingCfg<P>::D_TWIST ? lc : ly;
}
// mixed addition T + Q, Q = (x2, y2) affine (TIGHT < 2p): n = Y - y2 Z, m = X - x2 Z,
//     h = m^3 + Z n^2 - 2 X m^2,  X3 = m h,  Y3 = n (X m^2 - h) - m^3 Y,  Z3 = Z m^3;   constant term of the line: n x2 - m y2
// (T = +-Q and T = O do not occur for points of order r: the loop count is below r; points that are not of order r are refused)
template <class P>
ZK_HD void pair_add_step(Fu2<P>& X, Fu2<P>& Y, Fu2<P>& Z, const Fu2<P>& x2, const Fu2<P>& y2, const Fu<P>& yP, const Fu<P>& nxP, Fu2<P>& l0, Fu2<P>& l1,
                         Fu2<P>& l2) {
    typedef Fu2<P> F;
    const F n = fe_relax(fe_sub_k<2>(Y, ec_mul(y2, Z)));            // < 5p -> < 3p
    const F m = fe_relax(fe_sub_k<2>(X, ec_mul(x2, Z)));
    const F ly = f2_scale(m, yP);
    const F lx = f2_scale(n, nxP);
    const F lc = fe_relax(fe_sub_k<2>(ec_mul(n, x2), ec_mul(m, y2)));   // < 4p -> < 3p
    const F c = ec_sqr(n), d = ec_sqr(m);
    const F e = ec_mul(m, d), f = ec_mul(Z, c), g = ec_mul(X, d);   // < 2p
    const F h = fe_relax(fe_sub_k<4>(fe_add(e, f), fe_dbl(g)));     // 2g < 4p (a product is < 1.4p); < 8p -> < 3p
    const F t = ec_mul(n, fe_sub_k<4>(g, h));                       // g + 4p - h < 6p
    X = ec_mul(m, h);
    Y = fe_relax(fe_sub_k<2>(t, ec_mul(e, Y)));                     // < 4p -> < 3p
    Z = ec_mul(Z, e);
    l0 = PairingCfg<P>::D_TWIST ? ly : lc;
    l1 = lx;
    l2 = PairingCfg<P>::D_TWIST ? lc : ly;
}

// ---- admission: one lane per point.  Point i is read at raw + i stride + coord_off (NC x sz(Fq) bytes, canonical little-endian)
// with its flag byte at raw + i stride + flag_off (non-zero: the point at infinity, as in a proof record) and written, in the
// unsaturated limbs the pairing kernel reads, to out[i out_stride + out_off]; status likewise: PT_GOOD, inf_status for a flagged
// point (PT_INF: the pair contributes 1, the primitive's reading; PT_REFUSED: the verifiers', as the host verifier's), PT_REFUSED
// (off its curve or outside the r-torsion) or PT_NONCANON (a coordinate >= p: the caller's error).  neg: -P is written.  sat (may
// be null): the point as it was given, in the saturated Montgomery form, for the kernels that add it to something.
// BN254's G1 has cofactor 1: the curve test is the group test
struct AdmitJob {
    const uint8_t* raw;
    u64 stride, coord_off, flag_off;
    void* out;
    u64 out_stride, out_off;
    uint8_t* status;
    void* sat;
    int neg;
    uint8_t inf_status;
};
template <class P, bool G2>
__global__ void __launch_bounds__(64) k_pair_admit(AdmitJob j, u64 n, AdmitConsts<P> c) {
    typedef Fe<P> Fq;
    typedef typename std::conditional<G2, Fe2<P>, Fe<P>>::type F;
    typedef typename Unsat<F>::type U;
    constexpr int NC = G2 ? 4 : 2, SZ = 4 * P::N;
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<U>* out = (Aff<U>*)j.out + (i * j.out_stride + j.out_off);
    uint8_t* status = j.status + (i * j.out_stride + j.out_off);
    const uint8_t* rec = j.raw + i * j.stride + j.coord_off;
    Fq v[NC];
    bool canon = true;
    for (int q = 0; q < NC; ++q) {
        for (int w = 0; w < P::N; ++w) {
            const uint8_t* b = rec + q * SZ + 4 * w;
            v[q].v[w] = (u32)b[0] | (u32)b[1] << 8 | (u32)b[2] << 16 | (u32)b[3] << 24;
        }
        bool below = false;                                  // v < p, from the top word down
        for (int w = P::N - 1; w >= 0; --w) {
            if (v[q].v[w] != P::mod(w)) { below = v[q].v[w] < P::mod(w); break; }
        }
        canon = canon && below;
    }
    *out = Aff<U>::inf();
    if (j.sat) ((Aff<F>*)j.sat)[i] = Aff<F>::inf();
    if (j.raw[i * j.stride + j.flag_off] != 0) { *status = j.inf_status; return; }
    if (!canon) { *status = PT_NONCANON; return; }
    Aff<F> a;
    bool good;
    if constexpr (G2) {
        a = {{fe_to_mont(v[0]), fe_to_mont(v[1])}, {fe_to_mont(v[2]), fe_to_mont(v[3])}};
        const F rhs = fe_add(fe_mul(fe_sqr(a.x), a.x), c.b2), lhs = fe_sqr(a.y);
        good = fe_sub(lhs, rhs).is_zero();
    } else {
        a = {fe_to_mont(v[0]), fe_to_mont(v[1])};
        good = fe_sub(fe_sqr(a.y), fe_add(fe_mul(fe_sqr(a.x), a.x), c.b1)).is_zero();
    }
    if (good && (G2 || PairingCfg<P>::LOOP != 0)) good = xyzz_mul_limbs(Xyzz<F>::from_affine(a), c.r, 8).is_inf();
    if (!good) { *status = PT_REFUSED; return; }
    if (j.sat) ((Aff<F>*)j.sat)[i] = a;
    if (j.neg) a.y = fe_neg(a.y);
    *out = {fu_from_fe(a.x), fu_from_fe(a.y)};
    *status = PT_GOOD;
}

// ---- the verifiers' own kernels (cold: a handful of group operations per proof, in the saturated form and with the group law of ec.cuh)
// base[0] + sum_i input_i base[i + 1] for one proof per workgroup: lane t takes the inputs t, t + 64, ... (INPUT_CHUNK = 64 per
// round, any l), lane 0 adds the 64 partial sums.  inputs: l x 32 B per proof, canonical little-endian; an input >= r is the
// caller's error: *err takes the lowest (item l + index).  neg: the negated sum is written.  The sum O is a pair that contributes 1
static constexpr int INPUT_CHUNK = 64;
template <class P>
__global__ void __launch_bounds__(64) k_input_combination(const uint8_t* __restrict__ inputs, u64 l, const Aff<Fe<P>>* __restrict__ base, AdmitConsts<P> c, int neg,
                                                          Aff<Fu<P>>* out, u64 out_stride, u64 out_off, uint8_t* status, unsigned long long* err) {
    typedef Fe<P> Fq;
    ZK_DYN_SMEM(smem);
    Xyzz<Fq>* sh = (Xyzz<Fq>*)smem;
    const u64 item = blockIdx.x;
    const int t = (int)threadIdx.x;
    Xyzz<Fq> acc = Xyzz<Fq>::inf();
    for (u64 i = (u64)t; i < l; i += INPUT_CHUNK) {
        const uint8_t* b = inputs + (item * l + i) * 32;
        u32 k[8];
        for (int w = 0; w < 8; ++w) k[w] = (u32)b[4 * w] | (u32)b[4 * w + 1] << 8 | (u32)b[4 * w + 2] << 16 | (u32)b[4 * w + 3] << 24;
        bool below = false;
        for (int w = 7; w >= 0; --w) {
            if (k[w] != c.r[w]) { below = k[w] < c.r[w]; break; }
        }
        if (!below) { atomicMin(err, (unsigned long long)(item * l + i)); continue; }
        acc = xyzz_add(acc, xyzz_mul_limbs(Xyzz<Fq>::from_affine(base[i + 1]), k, 8));
    }
    sh[t] = acc;
    __syncthreads();
    if (t != 0) return;
    Xyzz<Fq> s = Xyzz<Fq>::from_affine(base[0]);
    for (int q = 0; q < INPUT_CHUNK; ++q) s = xyzz_add(s, sh[q]);
    Aff<Fq> a = xyzz_to_affine(s);
    const u64 o = item * out_stride + out_off;
    if (a.is_inf()) { out[o] = Aff<Fu<P>>::inf(); status[o] = PT_INF; return; }
    if (neg) a.y = fe_neg(a.y);
    out[o] = {fu_from_fe(a.x), fu_from_fe(a.y)};
    status[o] = PT_GOOD;
}
// the key's own points into the slots of every item: pair j of item i takes k1[g1_src[j]] / k2[g2_src[j]] (-1: the slot is a proof's)
struct PairFill { int g1_src[PAIR_LANES], g2_src[PAIR_LANES]; };
template <class P>
__global__ void __launch_bounds__(256) k_pair_fill(Aff<Fu<P>>* g1, Aff<Fu2<P>>* g2, uint8_t* st1, uint8_t* st2, u64 count, u32 npairs, const Aff<Fu<P>>* __restrict__ k1,
                                                    const Aff<Fu2<P>>* __restrict__ k2, PairFill f) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * npairs) return;
    const int j = (int)(i % npairs);
    if (f.g1_src[j] >= 0) { g1[i] = k1[f.g1_src[j]]; st1[i] = PT_GOOD; }
    if (f.g2_src[j] >= 0) { g2[i] = k2[f.g2_src[j]]; st2[i] = PT_GOOD; }
}
// GM17's fourth pair, per proof: (-(A + g_alpha), B + h_beta) from the admitted A and B (saturated form; the point at infinity where
// the proof's point was not admitted: the item is refused through A's and B's own slots in the second product)
template <class P>
__global__ void __launch_bounds__(64) k_gm17_sums(const Aff<Fe<P>>* __restrict__ a_sat, const Aff<Fe2<P>>* __restrict__ b_sat, Aff<Fe<P>> g_alpha, Aff<Fe2<P>> h_beta,
                                                   u64 count, Aff<Fu<P>>* g1, Aff<Fu2<P>>* g2, uint8_t* st1, uint8_t* st2, u64 out_stride, u64 out_off) {
    typedef Fe<P> Fq;
    typedef Fe2<P> Fq2;
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64 o = i * out_stride + out_off;
    const bool have = !a_sat[i].is_inf() && !b_sat[i].is_inf();
    Aff<Fq> s1 = Aff<Fq>::inf();
    Aff<Fq2> s2 = Aff<Fq2>::inf();
    if (have) {
        s1 = xyzz_to_affine(xyzz_add(Xyzz<Fq>::from_affine(a_sat[i]), Xyzz<Fq>::from_affine(g_alpha)));
        s2 = xyzz_to_affine(xyzz_add(Xyzz<Fq2>::from_affine(b_sat[i]), Xyzz<Fq2>::from_affine(h_beta)));
    }
    if (!have) { g1[o] = Aff<Fu<P>>::inf(); g2[o] = Aff<Fu2<P>>::inf(); st1[o] = PT_REFUSED; st2[o] = PT_REFUSED; return; }
    if (s1.is_inf()) { g1[o] = Aff<Fu<P>>::inf(); st1[o] = PT_INF; }
    else { g1[o] = {fu_from_fe(s1.x), fu_from_fe(fe_neg(s1.y))}; st1[o] = PT_GOOD; }
    if (s2.is_inf()) { g2[o] = Aff<Fu2<P>>::inf(); st2[o] = PT_INF; }
    else { g2[o] = {fu_from_fe(s2.x), fu_from_fe(s2.y)}; st2[o] = PT_GOOD; }
}

// ---- the pairing check: ok[item] = every point of the item admitted and prod_j e(P_j, Q_j) == 1 (pairs with a point at infinity
// contribute 1).  One workgroup of 64 = PAIR_ITEMS groups of PAIR_LANES; dynamic LDS: PAIR_ITEMS x PairLds.  Every loop bound is a
// constant of the launch, so every barrier is reached by all 64 lanes; the groups past `count` compute the last item again and
// write nothing.
// Registers of the final exponentiation: 0 f -> f1, 1 conj6(f) -> Frobenius^2(f1), 2 the norm -> 1 / f -> the running power,
// 3 the inverse norm -> f2.  Its products — four of the easy part, two per bit of the hard exponent — share ONE site of the Fq12
// product: the steps are numbered and the loop picks the operands.
template <class P>
__global__ void __launch_bounds__(64) k_pairing(const Aff<Fu<P>>* __restrict__ g1, const Aff<Fu2<P>>* __restrict__ g2, const uint8_t* __restrict__ st1,
                                                const uint8_t* __restrict__ st2, u64 count, u32 npairs, PairConsts<P> c, uint8_t* __restrict__ ok) {
    typedef Fu2<P> F;
    ZK_DYN_SMEM(smem);
    const int tid = (int)threadIdx.x, grp = tid / PAIR_LANES, k = tid % PAIR_LANES;
    PairLds<P>* L = (PairLds<P>*)smem + grp;
    const u64 item = (u64)blockIdx.x * PAIR_ITEMS + grp, item_c = item < count ? item : count - 1;
    const bool mine = (u32)k < npairs;
    const u64 idx = item_c * npairs + (mine ? (u32)k : 0u);
    const uint8_t s1 = st1[idx], s2 = st2[idx];
    const bool skip = s1 == PT_INF || s2 == PT_INF;
    L->bad[k] = (mine && (s1 >= PT_REFUSED || s2 >= PT_REFUSED)) ? 1u : 0u;
    const Fu<P> yP = g1[idx].y, nxP = fe_neg(g1[idx].x);
    F X = g2[idx].x, Y = g2[idx].y, Z = F::one();
    f12_set_one(L, 0, k);
    for (int i = c.loop_bits - 2; i >= 0; --i) {
        f12_mul(L, 0, 0, 0, k);                              // one squaring per loop bit, however many pairs
        const int phases = ((c.loop[i >> 5] >> (i & 31)) & 1) ? 2 : 1;
        for (int ph = 0; ph < phases; ++ph) {
            F l0 = F::zero(), l1 = F::zero(), l2 = F::zero();
            if (mine) {
                if (ph == 0) pair_dbl_step<P>(X, Y, Z, yP, nxP, c.b3, l0, l1, l2);
                else pair_add_step<P>(X, Y, Z, g2[idx].x, g2[idx].y, yP, nxP, l0, l1, l2);
            }
            for (u32 j = 0; j < npairs; ++j) {
                // (every lane is past the barrier that follows the last read of L->line)
                if ((u32)k == j) { L->line[0] = l0; L->line[1] = l1; L->line[2] = l2; L->skip = skip ? 1u : 0u; }
                __syncthreads();
                f12_mul_line(L, 0, 0, k, L->skip != 0);
            }
        }
    }
    const int nsteps = 4 + 2 * c.hard_bits;
    for (int s = 0; s < nsteps; ++s) {
        int d, a, b;
        if (s == 0) { f12_conj6(L, 1, 0, k); d = 2; a = 0; b = 1; }                       // the norm f conj6(f)
        else if (s == 1) { f12_inv_fq6(L, 3, 2, k); d = 2; a = 1; b = 3; }                // 1 / f
        else if (s == 2) { d = 0; a = 1; b = 2; }                                         // f1 = f^(p^6 - 1)
        else if (s == 3) { f12_frobenius(L, 1, 0, k, c); f12_frobenius(L, 1, 1, k, c); d = 3; a = 1; b = 0; }   // f2 = f1^(p^2 + 1)
        else {
            if (s == 4) f12_set_one(L, 2, k);
            const int bit = c.hard_bits - 1 - ((s - 4) >> 1);
            const bool sq = ((s - 4) & 1) == 0;
            if (!sq && !((c.hard[bit >> 5] >> (bit & 31)) & 1)) continue;
            d = 2; a = 2; b = sq ? 2 : 3;
        }
        f12_mul(L, d, a, b, k);
    }
    bool one = true;
    if (k < 6) {
        const F v = L->reg[2][k];
        const Fu<P> c0 = k == 0 ? fe_sub_k<4>(v.c0, Fu<P>::one()) : v.c0;   // < 7p
        one = fe_is_zero_modp(c0) && fe_is_zero_modp(v.c1);
    }
    L->vote[k] = one ? 1u : 0u;
    __syncthreads();
    if (k == 0 && item < count) {
        u32 good = 1;
        for (int q = 0; q < PAIR_LANES; ++q) good &= L->vote[q] & (L->bad[q] ^ 1u);
        ok[item] = (uint8_t)good;
    }
}

// ---- TEST ONLY (zkhip_tower_op): one Fq12 function per launch on raw limbs, through the same group functions and the same LDS
// layout as k_pairing.  a, b, out: count x 6 coefficients x 2 components x N limbs.  Op 2 multiplies a by the line whose values are
// b's coefficients at the line's positions (b's other coefficients are not read)
template <class P>
__global__ void __launch_bounds__(64) k_tower_op(const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out, u64 count, int op, PairConsts<P> c) {
    typedef Fu2<P> F;
    ZK_DYN_SMEM(smem);
    const int tid = (int)threadIdx.x, grp = tid / PAIR_LANES, k = tid % PAIR_LANES;
    PairLds<P>* L = (PairLds<P>*)smem + grp;
    const u64 item = (u64)blockIdx.x * PAIR_ITEMS + grp, item_c = item < count ? item : count - 1;
    constexpr int N = Fu<P>::N;
    if (k < 6) {
        const u32* pa = a + (item_c * 6 + k) * 2 * N;
        const u32* pb = b + (item_c * 6 + k) * 2 * N;
        F va, vb;
        for (int q = 0; q < N; ++q) { va.c0.v[q] = pa[q]; va.c1.v[q] = pa[N + q]; vb.c0.v[q] = pb[q]; vb.c1.v[q] = pb[N + q]; }
        L->reg[0][k] = va;
        L->reg[1][k] = vb;
        for (int t = 0; t < 3; ++t)
            if (line_pos<P>(t) == k) L->line[t] = vb;
    }
    __syncthreads();
    if (op == 0) f12_mul(L, 2, 0, 1, k);
    else if (op == 1) f12_mul(L, 2, 0, 0, k);
    else if (op == 2) f12_mul_line(L, 2, 0, k, false);
    else if (op == 3) f12_inverse(L, 2, 0, 1, 2, 3, k);
    else if (op == 4) f12_frobenius(L, 2, 0, k, c);
    else f12_conj6(L, 2, 0, k);
    if (k < 6 && item < count) {
        const F v = L->reg[2][k];
        u32* po = out + (item * 6 + k) * 2 * N;
        for (int q = 0; q < N; ++q) { po[q] = v.c0.v[q]; po[N + q] = v.c1.v[q]; }
    }
}

}  // namespace zk

// zkhip_vk: a verifying key whose points were admitted at load and are resident in the forms the kernels read
struct zkhip_vk {
    int curve = 0;
    int scheme = 0;               // 0 = Groth16, 1 = GM17
    zkhip_ctx* ctx = nullptr;
    u64 nq = 0;                   // points of gamma_abc / query: public inputs + 1
    zk::DBuf k1, k2;              // the fixed points, unsaturated: g16 {-alpha}, {beta, gamma, delta}; gm17 {g_alpha, -g_gamma}, {h, h_beta, h_gamma}
    zk::DBuf q_sat;               // gamma_abc / query, saturated Montgomery form (k_input_combination)
    std::vector<uint8_t> g1_sat, g2_sat;   // gm17: g_alpha and h_beta in the saturated form (k_gm17_sums takes them by value)
};

namespace zk {

// ---- host side: the numbers of a curve, the launches, the calls of the C ABI (included by core.cuh below the context) ----
// The verify calls run on a stream and in buffers of their own (zkhip_ctx::verify_stream, vfy) and touch no proof slot: they are
// allowed while a proof queue is open.
static inline Stream ctx_verify_stream(zkhip_ctx* ctx) {
    if (!ctx->verify_made) { ctx->verify_stream = stream_create(); ctx->verify_made = true; }
    return ctx->verify_stream;
}
template <class C>
struct PairingDev {
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef typename Fq::Params P;
    typedef PairingCfg<P> Cfg;
    struct Consts { PairConsts<P> pc; AdmitConsts<P> ac; };

    static void words(const Big& v, u32* out, size_t n) {
        require(v.size() <= n, ZKHIP_ERR_BAD_ARG, "pairing: a derived number does not fit its words");
        for (size_t i = 0; i < n; ++i) out[i] = i < v.size() ? v[i] : 0;
    }
    // xi, gamma_i = xi^(i (p - 1) / 6) and the twist's b' from p, r and xi, as verify.cpp's Pairing<P> derives them
    static Consts derive() {
        PairingNumbers num;
        if (const char* why = pairing_numbers<P>(num)) throw ApiError{ZKHIP_ERR_BAD_ARG, why};
        Consts o;
        memset(&o, 0, sizeof o);
        const Fq2 xi = {fe_from_u64<P>(Cfg::XI0), Fq::one()};
        Fq2 g1 = Fq2::one();
        for (int i = big_bits(num.frob) - 1; i >= 0; --i) {
            g1 = fe_sqr(g1);
            if (big_bit(num.frob, i)) g1 = fe_mul(g1, xi);
        }
        Fq2 g = Fq2::one();
        for (int i = 0; i < 6; ++i) { o.pc.gamma[i] = fu_from_fe(g); g = fe_mul(g, g1); }
        const Fq b1 = fe_from_u64<P>(Cfg::B);
        const Fq2 bb = {b1, Fq::zero()};
        const Fq2 b2 = Cfg::D_TWIST ? fe_mul(bb, fe_inv(xi)) : fe_mul(bb, xi);
        o.pc.b3 = fu_from_fe(fe_add(fe_dbl(b2), b2));
        words(num.loop, o.pc.loop, 4);
        o.pc.loop_bits = big_bits(num.loop);
        words(num.hard, o.pc.hard, 40);
        o.pc.hard_bits = big_bits(num.hard);
        o.ac.b1 = b1;
        o.ac.b2 = b2;
        words(num.r, o.ac.r, 8);
        return o;
    }
    static const Consts& consts() {
        static const Consts c = derive();
        return c;
    }
    static size_t lds_bytes() { return (size_t)PAIR_ITEMS * sizeof(PairLds<P>); }

    template <bool G2>
    static void admit(Stream s, const Consts& k, const AdmitJob& j, u64 n) {
        ZK_LAUNCH((k_pair_admit<P, G2>), dim3(blocks_for(n, 64)), dim3(64), 0, s, j, n, k.ac);
    }
    // zkhip_pairing_products
    static void products(zkhip_ctx* ctx, u64 count, u32 npairs, const uint8_t* g1, const uint8_t* g2, uint8_t* ok_out) {
        typedef Fu<P> U1;
        typedef Fu2<P> U2;
        const Consts& k = consts();
        Stream s = ctx_verify_stream(ctx);
        const u64 n = count * npairs;
        const size_t r1 = 2 * sizeof(Fq) + 1, r2 = 4 * sizeof(Fq) + 1;
        DBuf* v = ctx->vfy;
        v[0].ensure(n * r1); v[1].ensure(n * r2);
        v[2].ensure(n * sizeof(Aff<U1>)); v[3].ensure(n * sizeof(Aff<U2>));
        v[4].ensure(2 * n); v[5].ensure(count);
        dev_h2d(v[0].p, g1, n * r1, s);
        dev_h2d(v[1].p, g2, n * r2, s);
        uint8_t* st = ptr<uint8_t>(v[4]);
        admit<false>(s, k, AdmitJob{ptr<uint8_t>(v[0]), r1, 0, r1 - 1, v[2].p, 1, 0, st, nullptr, 0, PT_INF}, n);
        admit<true>(s, k, AdmitJob{ptr<uint8_t>(v[1]), r2, 0, r2 - 1, v[3].p, 1, 0, st + n, nullptr, 0, PT_INF}, n);
        ZK_LAUNCH((k_pairing<P>), dim3(blocks_for(count, PAIR_ITEMS)), dim3(64), lds_bytes(), s, ptr<Aff<U1>>(v[2]), ptr<Aff<U2>>(v[3]), st, st + n, count, npairs,
                  k.pc, ptr<uint8_t>(v[5]));
        std::vector<uint8_t> hst(2 * n), hok(count);
        dev_d2h(hst.data(), st, 2 * n, s);
        dev_d2h(hok.data(), v[5].p, count, s);
        stream_sync(s);
        for (u64 i = 0; i < n; ++i)          // the lowest item first: the host verifier's Error, and no verdict is written
            for (int grp = 0; grp < 2; ++grp)
                if (hst[grp * n + i] == PT_NONCANON)
                    throw ApiError{ZKHIP_ERR_PARSE, "pairing_products: item " + std::to_string(i / npairs) + ", pair " + std::to_string(i % npairs) + ": a coordinate of the " +
                                                        (grp ? "G2" : "G1") + " point is not below the field modulus"};
        memcpy(ok_out, hok.data(), count);
    }
    // zkhip_tower_op (tests only)
    static void tower_op(zkhip_ctx* ctx, int op, u64 count, const u32* a, const u32* b, u32* out) {
        const Consts& k = consts();
        Stream s = ctx_verify_stream(ctx);
        const size_t bytes = count * 12 * Fu<P>::N * sizeof(u32);
        DBuf* v = ctx->vfy;
        v[0].ensure(bytes); v[1].ensure(bytes); v[2].ensure(bytes);
        dev_h2d(v[0].p, a, bytes, s);
        dev_h2d(v[1].p, b, bytes, s);
        ZK_LAUNCH((k_tower_op<P>), dim3(blocks_for(count, PAIR_ITEMS)), dim3(64), lds_bytes(), s, ptr<u32>(v[0]), ptr<u32>(v[1]), ptr<u32>(v[2]), count, op, k.pc);
        dev_d2h(out, v[2].p, bytes, s);
        stream_sync(s);
    }
    // zkhip_vk_load_g16 / _gm17.  bytes: ark's VerifyingKey in the serialize_unchecked layout (the head of a proving.key) —
    // g16: alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1[]; gm17: h_g2, g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, query[];
    // a point is its coordinates, canonical little-endian, with ark's flag bits in the top of its last byte (bit 6: infinity).
    // Every point goes through the admission of the proof points; a key with a point that fails is refused
    static void vk_load(zkhip_ctx* ctx, int scheme, const uint8_t* bytes, size_t len, zkhip_vk* vk) {
        typedef Fu<P> U1;
        typedef Fu2<P> U2;
        const Consts& k = consts();
        Stream s = ctx_verify_stream(ctx);
        const size_t fq = sizeof(Fq), G1B = 2 * fq, G2B = 4 * fq, r1 = G1B + 1, r2 = G2B + 1;
        const int nf = scheme ? 2 : 1;
        const size_t fixed = nf * G1B + 3 * G2B;
        require(len >= fixed + 8, ZKHIP_ERR_PARSE, "verifying key: too short for its fixed points");
        const size_t g1_at[2] = {scheme ? G2B : 0, 2 * G2B + G1B};
        const size_t g2_at[3] = {scheme ? 0 : G1B, scheme ? G2B + G1B : G1B + G2B, scheme ? 2 * G2B + 2 * G1B : G1B + 2 * G2B};
        u64 nq = 0;
        memcpy(&nq, bytes + fixed, 8);
        require(nq >= 1 && nq <= (len - fixed - 8) / G1B, ZKHIP_ERR_PARSE, "verifying key: the input bases run past the end of the key (a truncated key?)");
        std::vector<uint8_t> h1((nf + nq) * r1), h2(3 * r2);
        auto put = [&](uint8_t* dst, const uint8_t* src, size_t nbytes) {
            memcpy(dst, src, nbytes);
            dst[nbytes] = (src[nbytes - 1] & 0x40) ? 1 : 0;      // ark's infinity flag; its other flag bit (0x80) is never set in this layout
            dst[nbytes - 1] &= 0xbf;                             // and stays part of the coordinate: set, the coordinate is not canonical
        };
        for (int i = 0; i < nf; ++i) put(&h1[i * r1], bytes + g1_at[i], G1B);
        for (u64 i = 0; i < nq; ++i) put(&h1[(nf + i) * r1], bytes + fixed + 8 + i * G1B, G1B);
        for (int i = 0; i < 3; ++i) put(&h2[i * r2], bytes + g2_at[i], G2B);
        DBuf* v = ctx->vfy;
        const u64 nst = nf + nq + 3;
        v[0].ensure(h1.size()); v[1].ensure(h2.size()); v[2].ensure(nq * sizeof(Aff<U1>)); v[4].ensure(nst);
        // (nothing a kernel of this call writes is freed while it may run: the two staging buffers are the context's, and the key's
        // own buffers — which the caller frees with the key if this throws — are only let go once the stream is idle)
        struct Drain {
            Stream s;
            ~Drain() { try { stream_sync(s); } catch (...) {} }
        } drain{s};
        DBuf &sat1 = v[5], &sat2 = v[6];
        sat1.ensure(sizeof(Aff<Fq>)); sat2.ensure(3 * sizeof(Aff<Fq2>));
        vk->k1.ensure(2 * sizeof(Aff<U1>)); vk->k2.ensure(3 * sizeof(Aff<U2>)); vk->q_sat.ensure(nq * sizeof(Aff<Fq>));
        dev_h2d(v[0].p, h1.data(), h1.size(), s);
        dev_h2d(v[1].p, h2.data(), h2.size(), s);
        uint8_t* st = ptr<uint8_t>(v[4]);
        const uint8_t* d1 = ptr<uint8_t>(v[0]);
        admit<false>(s, k, AdmitJob{d1, r1, 0, G1B, vk->k1.p, 1, 0, st, sat1.p, scheme ? 0 : 1, PT_REFUSED}, 1);
        if (scheme) admit<false>(s, k, AdmitJob{d1 + r1, r1, 0, G1B, vk->k1.p, 1, 1, st, nullptr, 1, PT_REFUSED}, 1);
        admit<false>(s, k, AdmitJob{d1 + nf * r1, r1, 0, G1B, v[2].p, 1, 0, st + nf, vk->q_sat.p, 0, PT_REFUSED}, nq);
        admit<true>(s, k, AdmitJob{ptr<uint8_t>(v[1]), r2, 0, G2B, vk->k2.p, 1, 0, st + nf + nq, sat2.p, 0, PT_REFUSED}, 3);
        std::vector<uint8_t> hst(nst);
        dev_d2h(hst.data(), st, nst, s);
        vk->g1_sat.resize(sizeof(Aff<Fq>)); vk->g2_sat.resize(sizeof(Aff<Fq2>));
        dev_d2h(vk->g1_sat.data(), sat1.p, sizeof(Aff<Fq>), s);
        dev_d2h(vk->g2_sat.data(), (const char*)sat2.p + sizeof(Aff<Fq2>), sizeof(Aff<Fq2>), s);
        stream_sync(s);
        for (u64 i = 0; i < nst; ++i)
            if (hst[i] != PT_GOOD) {
                static const char* const names[2][5] = {{"alpha", "", "beta", "gamma", "delta"}, {"g_alpha", "g_gamma", "h", "h_beta", "h_gamma"}};
                const std::string which = i < (u64)nf ? names[scheme][i] : i < nf + nq ? std::string(scheme ? "query[" : "gamma_abc[") + std::to_string(i - nf) + "]"
                                                                                       : names[scheme][2 + (i - nf - nq)];
                throw ApiError{ZKHIP_ERR_PARSE, "verifying key: " + which + (hst[i] == PT_NONCANON ? " has a coordinate that is not below the field modulus"
                                                                                                   : " is not a point of order r of its group (or is the point at infinity)")};
            }
        vk->nq = nq;
        vk->scheme = scheme;
    }

    // zkhip_verify_g16_batch / _gm17_batch
    static void verify(zkhip_ctx* ctx, const zkhip_vk* vk, u64 count, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok_out) {
        typedef Fu<P> U1;
        typedef Fu2<P> U2;
        const Consts& k = consts();
        Stream s = ctx_verify_stream(ctx);
        const bool gm = vk->scheme != 0;
        const size_t fq = sizeof(Fq), rec = 8 * fq + 3;
        const u64 l = vk->nq - 1, n4 = 4 * count, n2 = gm ? 2 * count : 0;
        DBuf* v = ctx->vfy;
        v[0].ensure(count * rec); v[1].ensure(std::max<u64>(1, count * l * 32));
        v[2].ensure(n4 * sizeof(Aff<U1>)); v[3].ensure(n4 * sizeof(Aff<U2>));
        v[4].ensure(2 * n4 + 2 * n2); v[5].ensure(2 * count); v[6].ensure(8);
        v[7].ensure(n2 * sizeof(Aff<U1>)); v[8].ensure(n2 * sizeof(Aff<U2>)); v[9].ensure(count * sizeof(Aff<Fq>)); v[10].ensure(count * sizeof(Aff<Fq2>));
        dev_h2d(v[0].p, proofs, count * rec, s);
        if (l) dev_h2d(v[1].p, inputs, count * l * 32, s);
        dev_memset(v[6].p, 0xff, 8, s);
        uint8_t *st1 = ptr<uint8_t>(v[4]), *st2 = st1 + n4, *sb1 = st2 + n4, *sb2 = sb1 + n2;
        const uint8_t* raw = ptr<uint8_t>(v[0]);
        Aff<U1>* g1 = ptr<Aff<U1>>(v[2]);
        Aff<U2>* g2 = ptr<Aff<U2>>(v[3]);
        unsigned long long* err = ptr<unsigned long long>(v[6]);
        const size_t comb_lds = (size_t)INPUT_CHUNK * sizeof(Xyzz<Fq>);
        PairFill f;
        for (int j = 0; j < PAIR_LANES; ++j) f.g1_src[j] = f.g2_src[j] = -1;
        if (!gm) {
            // e(A, B) e(-g_ic, gamma) e(-C, delta) e(-alpha, beta) == 1
            admit<false>(s, k, AdmitJob{raw, rec, 0, 8 * fq, g1, 4, 0, st1, nullptr, 0, PT_REFUSED}, count);
            admit<true>(s, k, AdmitJob{raw, rec, 2 * fq, 8 * fq + 1, g2, 4, 0, st2, nullptr, 0, PT_REFUSED}, count);
            admit<false>(s, k, AdmitJob{raw, rec, 6 * fq, 8 * fq + 2, g1, 4, 2, st1, nullptr, 1, PT_REFUSED}, count);
            ZK_LAUNCH((k_input_combination<P>), dim3((unsigned)count), dim3(64), comb_lds, s, ptr<uint8_t>(v[1]), l, ptr<Aff<Fq>>(vk->q_sat), k.ac, 1, g1, (u64)4, (u64)1, st1, err);
            f.g2_src[1] = 1; f.g2_src[2] = 2; f.g1_src[3] = 0; f.g2_src[3] = 0;
        } else {
            // e(g_alpha, h_beta) e(psi, h_gamma) e(C, h) e(-(A + g_alpha), B + h_beta) == 1   and   e(A, h_gamma) e(-g_gamma, B) == 1
            Aff<U1>* g1b = ptr<Aff<U1>>(v[7]);
            Aff<U2>* g2b = ptr<Aff<U2>>(v[8]);
            admit<false>(s, k, AdmitJob{raw, rec, 0, 8 * fq, g1b, 2, 0, sb1, v[9].p, 0, PT_REFUSED}, count);
            admit<true>(s, k, AdmitJob{raw, rec, 2 * fq, 8 * fq + 1, g2b, 2, 1, sb2, v[10].p, 0, PT_REFUSED}, count);
            admit<false>(s, k, AdmitJob{raw, rec, 6 * fq, 8 * fq + 2, g1, 4, 2, st1, nullptr, 0, PT_REFUSED}, count);
            ZK_LAUNCH((k_input_combination<P>), dim3((unsigned)count), dim3(64), comb_lds, s, ptr<uint8_t>(v[1]), l, ptr<Aff<Fq>>(vk->q_sat), k.ac, 0, g1, (u64)4, (u64)1, st1, err);
            Aff<Fq> g_alpha;
            Aff<Fq2> h_beta;
            memcpy(&g_alpha, vk->g1_sat.data(), sizeof g_alpha);
            memcpy(&h_beta, vk->g2_sat.data(), sizeof h_beta);
            ZK_LAUNCH((k_gm17_sums<P>), dim3(blocks_for(count, 64)), dim3(64), 0, s, ptr<Aff<Fq>>(v[9]), ptr<Aff<Fq2>>(v[10]), g_alpha, h_beta, count, g1, g2, st1, st2, (u64)4, (u64)3);
            f.g1_src[0] = 0; f.g2_src[0] = 1; f.g2_src[1] = 2; f.g2_src[2] = 0;
            PairFill fb;
            for (int j = 0; j < PAIR_LANES; ++j) fb.g1_src[j] = fb.g2_src[j] = -1;
            fb.g2_src[0] = 2; fb.g1_src[1] = 1;
            ZK_LAUNCH((k_pair_fill<P>), dim3(blocks_for(n2, 256)), dim3(256), 0, s, g1b, g2b, sb1, sb2, count, 2u, ptr<Aff<U1>>(vk->k1), ptr<Aff<U2>>(vk->k2), fb);
            ZK_LAUNCH((k_pairing<P>), dim3(blocks_for(count, PAIR_ITEMS)), dim3(64), lds_bytes(), s, g1b, g2b, sb1, sb2, count, 2u, k.pc, ptr<uint8_t>(v[5]) + count);
        }
        ZK_LAUNCH((k_pair_fill<P>), dim3(blocks_for(n4, 256)), dim3(256), 0, s, g1, g2, st1, st2, count, 4u, ptr<Aff<U1>>(vk->k1), ptr<Aff<U2>>(vk->k2), f);
        ZK_LAUNCH((k_pairing<P>), dim3(blocks_for(count, PAIR_ITEMS)), dim3(64), lds_bytes(), s, g1, g2, st1, st2, count, 4u, k.pc, ptr<uint8_t>(v[5]));
        std::vector<uint8_t> hst(2 * n4 + 2 * n2), hok(2 * count);
        unsigned long long herr = 0;
        dev_d2h(hst.data(), st1, hst.size(), s);
        dev_d2h(hok.data(), v[5].p, (gm ? 2 : 1) * count, s);
        dev_d2h(&herr, err, 8, s);
        stream_sync(s);
        // the host verifier's Error: a coordinate >= p or an input >= r; the lowest item is named and no verdict is written
        const u64 bad_input_item = herr == ~0ull ? ~(u64)0 : herr / l;
        for (u64 i = 0; i < count; ++i) {
            const uint8_t sa = gm ? hst[2 * n4 + 2 * i] : hst[4 * i], sb = gm ? hst[2 * n4 + n2 + 2 * i + 1] : hst[n4 + 4 * i], sc = hst[4 * i + 2];
            const char* pt = sa == PT_NONCANON ? "A" : sb == PT_NONCANON ? "B" : sc == PT_NONCANON ? "C" : nullptr;
            if (pt) throw ApiError{ZKHIP_ERR_PARSE, "verify: item " + std::to_string(i) + ": a coordinate of " + pt + " is not below the field modulus"};
            if (i == bad_input_item)
                throw ApiError{ZKHIP_ERR_PARSE, "verify: item " + std::to_string(i) + ": input " + std::to_string(herr % l) + " is not below the scalar field modulus"};
        }
        for (u64 i = 0; i < count; ++i) ok_out[i] = gm ? (hok[i] & hok[count + i]) : hok[i];
    }
};

}  // namespace zk
