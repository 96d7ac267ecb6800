"""The group law of zokrates_amd/csrc/ec.cuh, bind.cuh and kernels_msm.cuh, one function at a time, against the chord-and-tangent
law in affine coordinates over Python integers.

zkhip_group_op (include/zkhip.h) runs each function element by element and hands back the raw limbs.  One body: on the emulator
build in the CPU suite, on the GPU under `-m gpu`; three curves, both groups, both forms (0: the saturated words of the fixed-base
kernels and the host, 1: the unsaturated limbs of the MSM, fold and bind kernels).

Operands.  The XYZZ formulas are identities of rational functions in x = X/ZZ, y = Y/ZZZ under ZZ^3 = ZZZ^2, so an operand need
not lie on the curve.  X and Y take any limbs their written bound allows: the operand classes and generators of
tests/test_fieldu_contract.py (limbs at 2^B + 8, values next to every multiple of p below the bound, single-limb patterns, the
top-limb rule where the coordinate is the subtrahend of a sub<K>).  (ZZ, ZZZ) = (t^2, t^3) for some t; they reach an edge where the
edge has the square or cube root that yields t (over Fq2 component by component: t = (t0, 0), (0, t1), t1 = e / 2 t0).

Edge lists.  Form.pool keeps EVERY exact value of fc.boundary_operands in every spelling and thins only its random limb patterns
(N_PATTERN of 40); what is cut for time is N_RANDOM.  Form.named lists the values each coordinate must reach — 0, 1, the image
of 1, j p and j p +- 1 up to the bound, the bound less one, the top-limb cap — and build_cases asserts, before any call, that each
of them stands in X and in Y (each component) of an operand the function sees as FINITE.  An edge is not spent on an operand that
is then made infinite, nor a Y edge on a Y that is then zeroed.  The scalar multiplications (a few hundred elements) take the named
values in one spelling each; the other ops the whole lists.

Cases.  One operand is at an edge, the other derived from the reference point: another point (plain), the same point in another
representation (the doubling), its opposite (the cancellation; through `neg` in the ops that negate), a point with y = 0 (an
order-two "point": infinity), the point at infinity on either side.  One random case in eight is a pair of generator multiples.
The reference COUNTS the kinds before the call, in every run of 64 elements (a wavefront diverges) and in two uniform runs (all
doublings, all cancellations); nothing is assumed about which branch ran.

Checked on every result, exactly: infinite when and only when the reference is; X = x ZZ, Y = y ZZZ, ZZ^3 = ZZZ^2 mod p; every limb
below the top one <= 2^B + 8; every value below the bound ec.cuh writes for it.  Stored: X < 3p, Y < 4p, ZZ and ZZZ < 2p.  After
the mixed addition proper Y < 2p over G1 and < 3p over G2 where its sum is fused; after xyzz_neg_u Y < 3p.  Form 0: canonical.
Affine results: form 0 the reference's canonical Montgomery integer; form 1 (xyzz_to_affine_u ends in products, which aff_pack
then packs) the same residue, TIGHT, < 2p.

Scope left out, and why:
  - xyzz_add, xyzz_add_to, xyzz_mul_u32, xyzz_to_affine in form 1: they test for zero limb-wise, right on canonical values only; no
    kernel calls them on unsaturated limbs.
  - xyzz_neg_u, xyzz_to_affine_u, xyzz_mul_words and xyzz_add_from with neg over G2: the bind kernels, their only callers, are G1.
  - xyzz_madd_acc with neg in form 0; `neg` taken at run time by xyzz_madd_acc or xyzz_add_from: every call in the product passes
    a constant (ops madd_acc_neg and add_from_neg are the instantiations with `true`).
  - infinite bases of the mixed additions: their precondition, every caller filters them.
  - the accumulation kernel's own hot path.  Op madd_hot holds xyzz_madd_begin / xyzz_madd_finish as ec.cuh defines them, but no
    kernel calls those: k_msm_accum carries an inlined copy which over G1 differs (X1 un-reduced below 10p, sub<16> for Pp, no
    fe_relax on X3).  That copy stays covered through MSMs and proofs only.

Found by this file, written where it belongs (the bounds comment and the comment at Y3 in ec.cuh): a stored Y is a subtrahend too
— over Fq2 every doubling negates the second component of 2Y against 8p, and a Y.c1 within 2^(B (N - 1)) of 4p made the doubling
return another point on BLS12-377; no producer leaves such a Y — and the cold Fq2 kernels of the BLS curves leave the mixed
addition's Y below 4p, not 3p (3.003p on the device)."""
import random

import numpy as np
import pytest

import bls377_ref
import test_fieldu_contract as fc
from oracle.fields import BLS12_381, BN254, FqOps
from zokrates_amd import native

from emu_util import emu_library

CURVES = [(BN254, 0, fc.FIELDS[0]), (BLS12_381, 1, fc.FIELDS[1]), (bls377_ref.CURVE, 2, fc.FIELDS[2])]
N_RANDOM = 1024          # seeded random cases per op, after the edge lists (what is cut when time is short: never the edge lists)
N_LADDER = 256           # elements of the 253 to 255-bit ladder, at least
N_SMALL_MUL = 512        # elements of the 32-bit multiplications, at least
N_PATTERN = 8            # random limb patterns per class beside the five fixed ones (fc.boundary_operands draws 40 for one operation)

# op -> (forms, groups, a, b, neg (False, True: per element through the flag, "always": the op's constant), kinds, bound of a result's Y
# in the plain case (p))
MADD_KINDS = ["plain", "a_inf", "dbl", "cancel", "order2"]
ADD_KINDS = ["plain", "a_inf", "b_inf", "both_inf", "dbl", "cancel", "order2"]
OPS = {
    "madd_acc": ((0, 1), (1, 2), "xyzz", "aff", False, MADD_KINDS, 3),
    "madd_cold": ((1,), (1, 2), "xyzz", "aff", False, MADD_KINDS, 3),
    "madd_hot": ((1,), (1, 2), "xyzz", "aff", True, ["plain"], 3),
    "add_acc": ((1,), (1, 2), "xyzz", "xyzz", False, ADD_KINDS, 4),
    "add_from": ((1,), (1, 2), "xyzz", "xyzz", False, ADD_KINDS, 4),
    "add": ((0,), (1, 2), "xyzz", "xyzz", False, ADD_KINDS, 4),
    "add_to": ((0,), (1, 2), "xyzz", "xyzz", False, ADD_KINDS, 4),
    "dbl": ((0, 1), (1, 2), "xyzz", None, False, ["plain", "inf", "order2"], 4),
    "dbl_inl": ((1,), (1, 2), "xyzz", None, False, ["plain", "inf", "order2"], 4),
    "dbl_acc": ((1,), (1, 2), "xyzz", None, False, ["plain", "inf", "order2"], 4),
    "dbl_affine": ((1,), (1, 2), "aff", None, False, ["plain", "inf", "order2"], 4),
    "dbl_affine_hot": ((1,), (1, 2), "aff", None, False, ["plain", "inf", "order2"], 4),
    "neg_u": ((1,), (1,), "xyzz", None, False, ["plain", "inf"], 3),
    "to_affine": ((0,), (1, 2), "xyzz", None, False, ["plain", "inf"], None),
    "to_affine_u": ((1,), (1,), "xyzz", None, False, ["plain", "inf"], None),
    "mul_words": ((1,), (1,), "xyzz", None, False, ["plain", "inf", "order2", "k0"], 4),
    "mul_u32": ((0,), (1, 2), "xyzz", None, False, ["plain", "inf", "order2", "k0"], 4),
    "mul_small": ((1,), (1, 2), "xyzz", None, False, ["plain", "inf", "order2", "k0"], 4),
    "madd_acc_neg": ((1,), (1, 2), "xyzz", "aff", "always", MADD_KINDS, 3),
    "add_from_neg": ((1,), (1,), "xyzz", "xyzz", "always", ADD_KINDS, 4),
}
AFFINE_RESULT = ("to_affine", "to_affine_u")
MULS = ("mul_words", "mul_u32", "mul_small")
# Operand classes (kind, K, cap): fc's class (kind, K) with the value below cap p.  Stored points: X < 3p, Y < 4p, ZZ, ZZZ < 2p; affine
# coordinates canonical-sized.  Where the function subtracts the coordinate (sub<K>), the class is the subtrahend's ("S": the top-limb
# rule of fieldu.cuh:17-24): X1 and Y1 of the mixed additions (Pp = U2 - X1, R = S2 - Y1 against 4p), the base's y (negated against 2p),
# Y of a negated point (xyzz_y_of, xyzz_neg_u: against 4p).
STORED = [("T", 3, 3), ("T", 4, 4), ("T", 2, 2), ("T", 2, 2)]
MADD_A = [("S", 4, 3), ("S", 4, 4), ("T", 2, 2), ("T", 2, 2)]
AFF = [("T", 2, 1), ("S", 2, 1)]
# Over Fq2 every doubling squares U = 2Y, and the square negates U's second component against 8p (fieldu.cuh fu2_sqr_inl): there Y is a
# subtrahend too, top limb <= (4p)_top - 2.  (A Y.c1 within 2^(B (N - 1)) of 4p gave a wrong ZZ3 on BLS12-377; no producer leaves
# one: see the bounds comment in ec.cuh.)
STORED_YSUB = [("T", 3, 3), ("S", 4, 4), ("T", 2, 2), ("T", 2, 2)]
CLASSES = {
    "madd_acc": (MADD_A, AFF), "madd_cold": (MADD_A, AFF), "madd_hot": (MADD_A, AFF), "madd_acc_neg": (MADD_A, AFF),
    "add_from_neg": (STORED, STORED_YSUB),       # (without neg, b's Y only meets products over G1: the default)
    "neg_u": ([("T", 3, 3), ("S", 4, 3), ("T", 2, 2), ("T", 2, 2)], None),
    "dbl_affine": (AFF, None), "dbl_affine_hot": (AFF, None),
}
CLASSES_G2 = dict(CLASSES, add_from=(STORED, STORED_YSUB), add_acc=(STORED_YSUB, STORED), dbl=(STORED_YSUB, None), dbl_inl=(STORED_YSUB, None), dbl_acc=(STORED_YSUB, None),
                  mul_small=(STORED_YSUB, None))


# ---------------------------------------------------------------- fields, roots, the reference
def nth_root(a, n, p):
    """an n-th root of a mod p (n = 2 or 3), or None: through the n-Sylow subgroup where n divides p - 1 (Pohlig-Hellman digits)"""
    a %= p
    if a == 0:
        return 0
    if (p - 1) % n:
        return pow(a, pow(n, -1, p - 1), p)
    if pow(a, (p - 1) // n, p) != 1:
        return None
    s, m = 0, p - 1
    while m % n == 0:
        s, m = s + 1, m // n
    k = pow(n, -1, m)
    x, b = pow(a, k, p), pow(a, n * k - 1, p)           # x^n = a b, b in the subgroup of order n^s
    g = 2
    while pow(g, (p - 1) // n, p) == 1:
        g += 1
    c = pow(g, m, p)
    cinv, w = pow(c, -1, p), pow(c, n ** (s - 1), p)
    j = 0
    for i in range(s):
        t = pow(b * pow(cinv, j, p) % p, n ** (s - 1 - i), p)
        d, u = 0, 1
        while u != t:
            u, d = u * w % p, d + 1
            assert d < n
        j += d * n ** i
    assert j % n == 0
    r = x * pow(cinv, j // n, p) % p
    assert pow(r, n, p) == a
    return r


class Fq(FqOps):
    def inv(self, a):                  # (the extended Euclid of pow: a tenth of the oracle's a^(p-2))
        return pow(a, -1, self.q)


class Fq2(bls377_ref.Fq2Beta):
    def inv(self, a):
        n = pow((a[0] * a[0] + self.beta * a[1] * a[1]) % self.q, -1, self.q)
        return (a[0] * n % self.q, (-a[1]) * n % self.q)


class Form:
    """one (curve, group, form): the limb layout, the coordinate field, and the generator's multiples"""

    def __init__(self, C, cid, fu, group, form):
        self.C, self.cid, self.group, self.form, self.p = C, cid, group, form, C.q
        self.f = fu if form == 1 else fc.Field(fu.name + "/words", C.q, 32, C.fq_bytes // 4, True, fu.beta)
        self.Rinv = pow(self.f.R, -1, self.p)
        self.K = Fq(self.p) if group == 1 else Fq2(self.p, fu.beta)
        self.lo_max = (1 << fu.B) + 8 if form == 1 else (1 << 32) - 1
        self.gen = C.g1 if group == 1 else C.g2
        self._pools = {}

    # an element of the coordinate field: a list of `group` limb lists <-> its residue (int, or a pair)
    def res(self, el):
        v = [self.f.val(l) * self.Rinv % self.p for l in el]
        return v[0] if self.group == 1 else (v[0], v[1])

    def comps(self, m):
        return [m] if self.group == 1 else list(m)

    def is_zero_limbs(self, el):
        return all(x == 0 for l in el for x in l)

    def admissible(self, cls, l):
        if self.form == 0:
            return self.f.val(l) < self.p
        return fc.admissible(self.f, cls[:2], l) and self.f.val(l) < cls[2] * self.p

    def named(self, cls):
        """The VALUES every coordinate of the class must reach in a finite operand (asserted before the call): 0, 1, the Montgomery
        image of 1, every multiple of p below the bound and its two neighbours, the bound less one, and for a subtrahend the two
        values at the top-limb cap."""
        f, p = self.f, self.p
        if self.form == 0:
            return {0, 1, p - 1, f.R % p}
        bound = cls[2] * p
        v = {0, 1, f.R % p, bound - 1}
        for j in range(1, cls[2] + 1):
            v.update((j * p - 1, j * p, j * p + 1))
        top_cap = fc.limit_of(f, cls[:2])[1]
        if top_cap is not None:
            v.update((min(bound - 1, ((top_cap + 1) << f.top_shift) - 1), top_cap << f.top_shift))
        return {x for x in v if x < bound and self.admissible(cls, f.split(x))}

    def pool(self, cls):
        """The edge operands of a class: ALL of fc.boundary_operands' exact values, in every spelling (the named values among them),
        and its limb patterns — the five fixed ones and N_PATTERN random ones (thinned from 40) under every top limb of interest.
        Nothing is sampled away afterwards."""
        key = cls if self.form == 1 else "W"
        if key not in self._pools:
            f, p = self.f, self.p
            if self.form == 1:
                out = [l for l in fc.boundary_operands(f, cls[:2], random.Random("pool/%s/%r" % (f.name, cls)), n_pattern=N_PATTERN) if f.val(l) < cls[2] * p]
            else:      # canonical words: Montgomery images at the edges of the value and of every word
                e = {0, 1, 2, p - 1, p - 2, (p - 1) // 2, f.R % p, (f.R % p) - 1, (1 << (p.bit_length() - 1)) - 1}
                for k in range(f.N):
                    e.update((0xffffffff << (32 * k), 1 << (32 * k), (1 << (32 * k)) - 1, (1 << (32 * k)) + 1))
                out = [f.split(x) for x in sorted(e) if 0 <= x < p]
            assert self.named(cls) <= {f.val(l) for l in out}, (cls, "a named value is missing from the edge list")
            self._pools[key] = out
        return self._pools[key]

    def random_limbs(self, cls, rnd):
        if self.form == 0:
            return self.f.split(rnd.randrange(self.p))
        while True:
            l = fc.random_operand(self.f, cls[:2], rnd)
            if self.f.val(l) < cls[2] * self.p:
                return l

    def spell(self, m, cls, rnd):
        """limbs of class `cls` for the residue m: its Montgomery image plus a multiple of p, in one of its TIGHT spellings"""
        f = self.f
        e = m * f.R % self.p
        if self.form == 0:
            return f.split(e)
        js = list(range(cls[2]))
        rnd.shuffle(js)
        for j in js:
            l = f.split(e + j * self.p)
            if rnd.random() < 0.5:
                alts = fc.respell(f, l, self.lo_max, rnd)
                if alts:
                    l = rnd.choice(alts)
            if self.admissible(cls, l):
                return l
        raise AssertionError(("no spelling", cls))

    def spell_el(self, m, cls, rnd):
        return [self.spell(c, cls, rnd) for c in self.comps(m)]

    def random_res(self, rnd, nonzero=True):
        while True:
            m = rnd.randrange(self.p) if self.group == 1 else (rnd.randrange(self.p), rnd.randrange(self.p))
            if not nonzero or not self.K.is_zero(m):
                return m


def ref_add(K, P, Q):
    """chord and tangent, affine, a = 0; None is the point at infinity"""
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        assert y1 == y2 or K.is_zero(K.add(y1, y2)), "equal x and y2 != +-y1: not a pair of points"
        if y1 != y2 or K.is_zero(y1):
            return None
        x1x1 = K.mul(x1, x1)
        lam = K.mul(K.add(K.add(x1x1, x1x1), x1x1), K.inv(K.add(y1, y1)))
    else:
        lam = K.mul(K.sub(y2, y1), K.inv(K.sub(x2, x1)))
    x3 = K.sub(K.sub(K.mul(lam, lam), x1), x2)
    return x3, K.sub(K.mul(lam, K.sub(x1, x3)), y1)


def ref_neg(K, P):
    return None if P is None else (P[0], K.neg(P[1]))


def ref_mul(K, k, P):
    r = None
    for i in range(k.bit_length() - 1, -1, -1):
        r = ref_add(K, r, r)
        if k >> i & 1:
            r = ref_add(K, r, P)
    return r


def kind_of(K, A, B):
    """what the reference says about A + B"""
    if A is None or B is None:
        return "both_inf" if A is None and B is None else "a_inf" if A is None else "b_inf"
    if A[0] != B[0]:
        return "plain"
    if A[1] == B[1]:
        return "order2" if K.is_zero(A[1]) else "dbl"
    return "cancel"


# ---------------------------------------------------------------- operands
def point_of(fm, op_limbs, kind):
    """the affine point an operand's limbs stand for (kind: "xyzz" or "aff")"""
    K = fm.K
    if kind == "aff":
        if fm.is_zero_limbs(op_limbs[0]) and fm.is_zero_limbs(op_limbs[1]):
            return None
        return fm.res(op_limbs[0]), fm.res(op_limbs[1])
    if fm.is_zero_limbs(op_limbs[2]):
        return None
    zz, zzz = fm.res(op_limbs[2]), fm.res(op_limbs[3])
    return K.mul(fm.res(op_limbs[0]), K.inv(zz)), K.mul(fm.res(op_limbs[1]), K.inv(zzz))


def from_point(fm, P, kind, classes, rnd, t=None):
    """an operand for the point P: affine, or XYZZ over a random t (its coordinates spelled at random within their classes)"""
    K = fm.K
    if kind == "aff":
        return [fm.spell_el(P[0], classes[0], rnd), fm.spell_el(P[1], classes[1], rnd)]
    t = t if t is not None else (K.one if rnd.random() < 0.1 else fm.random_res(rnd))
    t2 = K.mul(t, t)
    t3 = K.mul(t2, t)
    return [fm.spell_el(m, c, rnd) for m, c in zip((K.mul(P[0], t2), K.mul(P[1], t3), t2, t3), classes)]


def zz_edges(fm, classes, rnd):
    """(t, slot, component, limbs): values of t for which ZZ (slot 2) or ZZZ (slot 3) has exactly these edge limbs in one component"""
    f, p, K = fm.f, fm.p, fm.K
    out = []
    for slot in (2, 3):
        pool = fm.pool(classes[slot])
        pool = pool[:: max(1, len(pool) // 90)]
        for l in pool:
            m = f.val(l) * fm.Rinv % p
            if m == 0:
                continue
            n = slot          # ZZ = t^2, ZZZ = t^3
            if fm.group == 1:
                r = nth_root(m, n, p)
                if r is not None:
                    out.append((r, slot, 0, l))
                continue
            beta = f.beta
            r = nth_root(m, n, p)
            if r is not None:
                out.append(((r, 0), slot, 0, l))                   # t = (t0, 0): t^n = (t0^n, 0)
            if slot == 2:
                r = nth_root(-m * pow(beta, -1, p), 2, p)          # t = (0, t1): t^2 = (-beta t1^2, 0)
                if r is not None:
                    out.append(((0, r), 2, 0, l))
                t0 = rnd.randrange(1, p)                           # 2 t0 t1 = e
                out.append(((t0, m * pow(2 * t0, -1, p) % p), 2, 1, l))
            else:
                r = nth_root(-m * pow(beta, -1, p), 3, p)          # t = (0, t1): t^3 = (0, -beta t1^3)
                if r is not None:
                    out.append(((0, r), 3, 1, l))
    for t, slot, comp, l in out:
        tn = K.mul(K.mul(t, t), t) if slot == 3 else K.mul(t, t)
        assert fm.comps(tn)[comp] == f.val(l) * fm.Rinv % p
    return out


def edge_plan(fm, which, kind, classes, rnd, named_only=False):
    """The edge operands of one argument, as (which, slot, component, limbs, t): every coordinate's pool in every component.
    named_only (the scalar multiplications, whose lists are a few hundred elements): the named values, one spelling each, and a
    fifth of the ZZ / ZZZ edges."""
    plan = []
    for slot in (0, 1):
        for comp in range(fm.group):
            pool = fm.pool(classes[slot])
            if named_only:
                first = {}
                for l in pool:
                    first.setdefault(fm.f.val(l), l)
                pool = [first[v] for v in sorted(fm.named(classes[slot]))]
            plan += [(which, slot, comp, l, None) for l in pool]
    if kind == "xyzz":
        zz = [(which, slot, comp, l, t) for t, slot, comp, l in zz_edges(fm, classes, rnd)]
        plan += zz[::5] if named_only else zz
    return plan


def edge_operand(fm, kind, classes, edge, rnd, y_zero=False):
    """an operand with one coordinate component at the given edge limbs and everything else random within its class"""
    _, slot, comp, limbs, t = edge
    K = fm.K
    if kind == "aff":
        el = [[fm.random_limbs(classes[s], rnd) for _ in range(fm.group)] for s in (0, 1)]
    else:
        t = t if t is not None else fm.random_res(rnd)
        t2 = K.mul(t, t)
        el = [[fm.random_limbs(classes[s], rnd) for _ in range(fm.group)] for s in (0, 1)]
        el += [fm.spell_el(t2, classes[2], rnd), fm.spell_el(K.mul(t2, t), classes[3], rnd)]
    if y_zero:
        el[1] = fm.spell_el(K.zero, classes[1], rnd)
    if not (y_zero and slot == 1 and fm.f.val(limbs) % fm.p):      # (a Y edge that is itself 0 mod p stays under y = 0)
        el[slot][comp] = list(limbs)
    return el


def curve_points(fm, n=24):
    pts, P = [], None
    for _ in range(n):
        P = ref_add(fm.K, P, fm.gen)
        pts.append(P)
    return pts


def build_cases(fm, op):
    """(a, b, flags, scalars, kinds wanted): operand limbs per element, in the order they are sent"""
    forms, groups, akind, bkind, takes_neg, kinds, _ = OPS[op]
    ca, cb = (CLASSES_G2 if fm.group == 2 and fm.form == 1 else CLASSES).get(op, (STORED, STORED))
    if akind == "aff":
        ca = AFF
    rnd = random.Random("group_law/%s/%d/%d/%s" % (fm.C.name, fm.group, fm.form, op))
    K = fm.K
    on_curve = curve_points(fm)
    muls = op in MULS
    plan = edge_plan(fm, "a", akind, ca, rnd, muls)
    if bkind:
        plan += edge_plan(fm, "b", bkind, cb, rnd, muls)
    rnd.shuffle(plan)
    n_random = max(0, (N_LADDER if op == "mul_words" else N_SMALL_MUL) - len(plan)) if muls else N_RANDOM
    exc = [k for k in kinds if k != "plain"]

    def kind_at(i):      # every run of 64 holds every kind
        if bkind:
            return "plain" if i % 2 == 0 or not exc else exc[(i // 2) % len(exc)]
        return exc[(i // 8) % len(exc)] if i % 8 == 7 and exc else "plain"

    def suits(kind, edge):
        """an edge is only spent on an element that keeps it: not on an operand about to be made infinite, not on a Y about to be zeroed"""
        which, slot, _, limbs, _ = edge
        if kind in ("inf", "both_inf") or kind == which + "_inf":
            return False
        return kind != "order2" or slot != 1 or fm.f.val(limbs) % fm.p == 0
    A, Bs, flags, scal = [], [], [], []
    zero_el = [[0] * fm.f.N for _ in range(fm.group)]
    def build_one(kind, edge):
        fl = 0
        neg = takes_neg == "always" or (takes_neg and rnd.random() < 0.5)
        true_points = edge is None and rnd.random() < 0.125
        rand_pt = lambda: rnd.choice(on_curve) if true_points else (fm.random_res(rnd, False), fm.random_res(rnd))
        k = 0
        if not bkind:                                    # ---- one operand
            y_zero = kind == "order2"
            if edge is not None:
                a = edge_operand(fm, akind, ca, edge, rnd, y_zero)
            else:
                P = rand_pt()
                a = from_point(fm, (P[0], K.zero) if y_zero else P, akind, ca, rnd)
            if kind == "inf":
                if rnd.random() < 0.5:
                    fl |= 2
                elif akind == "aff":
                    a = [zero_el, zero_el]
                else:
                    a[2] = zero_el
            b = a
            if op in MULS:
                if op == "mul_words":
                    r = fm.C.r
                    k = rnd.choice([rnd.randrange(1 << 252, min(r, 1 << 255)), rnd.randrange(1 << 252, min(r, 1 << 255)), rnd.randrange(1 << 252, min(r, 1 << 255)), r - 1,
                                    rnd.randrange(1, 16), int("55" * 32, 16) >> 3, int("aa" * 32, 16) >> 3, (1 << 253) - 1, 1 << 252, 3 << 250, rnd.randrange(1 << 64)])
                else:
                    k = rnd.choice([1, 2, 3, 255, 256, 257, rnd.randrange(1, 512), rnd.randrange(1, 512), rnd.randrange(1 << 16), 0x80000000, 0xffffffff,
                                    rnd.randrange(1 << 32)])
                if kind == "k0":
                    k = 0
        else:                                            # ---- two operands
            which = edge[0] if edge is not None else rnd.choice("ab")
            ekind, ecls, dkind, dcls = (akind, ca, bkind, cb) if which == "a" else (bkind, cb, akind, ca)
            y_zero = kind == "order2"
            if edge is not None:
                e_op = edge_operand(fm, ekind, ecls, edge, rnd, y_zero)
            else:
                P = rand_pt()
                e_op = from_point(fm, (P[0], K.zero) if y_zero else P, ekind, ecls, rnd)
            P = point_of(fm, e_op, ekind)
            if P is None:                                # (an affine edge operand whose x and y are both all-zero limbs)
                P = rand_pt()
                e_op = from_point(fm, P, ekind, ecls, rnd)
            if kind in ("dbl", "order2"):
                Q = ref_neg(K, P) if neg else P
            elif kind == "cancel":
                Q = P if neg else ref_neg(K, P)
            else:
                Q = rand_pt()
                while Q[0] == P[0]:
                    Q = rand_pt()
            d_op = from_point(fm, Q, dkind, dcls, rnd)
            a, b = (e_op, d_op) if which == "a" else (d_op, e_op)
            for side, bit, okind in (("a", 2, akind), ("b", 4, bkind)):
                if kind == side + "_inf" or kind == "both_inf":
                    o = a if side == "a" else b
                    if rnd.random() < 0.5:
                        fl |= bit
                    elif okind == "aff":
                        o[0], o[1] = zero_el, zero_el
                    else:
                        o[2] = zero_el
        if akind == "aff":
            a = a + [zero_el, zero_el]
        if bkind == "aff":
            b = b + [zero_el, zero_el]
        if not bkind:
            b = a
        return a, b, fl | (1 if neg else 0), k

    want, seen, sched = [], [], []
    i = 0
    while plan or n_random > 0 or i % 64:
        assert i < 60000, ("edges that no element takes", plan[:3])
        kind = kind_at(i)
        i += 1
        sched.append(kind)
        # the last edge of the plan that suits the kind; one that turns the case into another kind all the same (y = 0 under a doubling,
        # say) goes back into the plan for an element it suits, and this element is built without an edge
        at = next((q for q in range(len(plan) - 1, -1, -1) if suits(kind, plan[q])), None)
        edge = plan.pop(at) if at is not None else None
        if not plan and edge is None:
            n_random -= 1
        for attempt in ([edge, None] if edge is not None else [None]):
            a, b, fl, k = build_one(kind, attempt)
            w, sk = classify(fm, op, a, b, fl, k)
            if sk == kind:
                break
            if attempt is not None:
                plan.insert(rnd.randrange(len(plan) + 1), attempt)
        A.append(a)
        Bs.append(b)
        flags.append(fl)
        scal.append(k)
        want.append(w)
        seen.append(sk)
    if bkind and "dbl" in kinds:      # the branch taken by a whole wavefront
        for kind in ["dbl"] * 64 + ["cancel"] * 64:
            a, b, fl, k = build_one(kind, None)
            w, sk = classify(fm, op, a, b, fl, k)
            sched.append(kind); A.append(a); Bs.append(b); flags.append(fl); scal.append(k); want.append(w); seen.append(sk)
    # every named value of every coordinate (X, Y; each component) stands in an operand the function sees as finite
    for side, okind, cls, ops_ in (("a", akind, ca, A), ("b", bkind, cb, Bs)):
        if not okind or (side == "b" and not bkind):
            continue
        finite = [o for o, fl in zip(ops_, flags) if not fl & (2 if side == "a" else 4) and point_of(fm, o, okind) is not None]
        for slot in (0, 1):
            for comp in range(fm.group):
                reached = {fm.f.val(o[slot][comp]) for o in finite}
                missing = fm.named(cls[slot]) - reached
                assert not missing, (op, side, slot, comp, [x / fm.p for x in sorted(missing)])
    return A, Bs, flags, scal, sched, want, seen


def to_array(fm, ops):
    return np.array([[[l for l in c] for c in o] for o in ops], dtype=np.uint32)


# ---------------------------------------------------------------- the test
_ctx = {}


@pytest.fixture(scope="module")
def contexts():
    def get(backend):
        if backend not in _ctx:
            c = native.Context(0, emu_library()) if backend == "emu" else native.Context(0)
            d = c.describe()
            assert ("EMULATOR" in d) == (backend == "emu") and (backend == "emu" or "gfx950" in d), d
            _ctx[backend] = c
        return _ctx[backend]
    yield get
    for c in _ctx.values():
        c.close()
    _ctx.clear()


_forms = {}
_cases = {}


def form_of(ci, group, form):
    key = (ci, group, form)
    if key not in _forms:
        C, cid, fu = CURVES[ci]
        _forms[key] = Form(C, cid, fu, group, form)
    return _forms[key]


def classify(fm, op, a, b, fl, k):
    """the reference's answer for one element, and what the reference says the element is"""
    forms, groups, akind, bkind, takes_neg, kinds, _ = OPS[op]
    K = fm.K
    P = None if fl & 2 else point_of(fm, a, akind)
    if bkind:
        Q = None if fl & 4 else point_of(fm, b, bkind)
        if fl & 1:
            Q = ref_neg(K, Q)
        return ref_add(K, P, Q), kind_of(K, P, Q)
    seen = "inf" if P is None else "k0" if op in MULS and k == 0 else "order2" if "order2" in kinds and K.is_zero(P[1]) else "plain"
    if op.startswith("dbl"):
        return ref_add(K, P, P), seen
    if op == "neg_u":
        return ref_neg(K, P), seen
    if op in AFFINE_RESULT:
        return P, seen
    return ref_mul(K, k, P), seen


def check_element(fm, op, got, want, kind, what):
    """one result (4 coordinates x components x limbs) against the reference point"""
    f, p, K = fm.f, fm.p, fm.K
    y_bound = OPS[op][6]
    el = [[[int(x) for x in comp] for comp in coord] for coord in got]
    if op in AFFINE_RESULT:
        assert fm.is_zero_limbs(el[2]) and fm.is_zero_limbs(el[3]), what
        if want is None:
            assert fm.is_zero_limbs(el[0]) and fm.is_zero_limbs(el[1]), ("infinity expected", what)
            return
        for c, w in zip(el[:2], want):
            for limbs, wc in zip(c, fm.comps(w)):
                assert all(x <= fm.lo_max for x in limbs[:-1]), ("limb bound", what)
                if fm.form == 0:
                    assert f.val(limbs) == wc * f.R % p, ("canonical value", what)
                else:
                    assert f.val(limbs) % p == wc * f.R % p and f.val(limbs) < 2 * p, ("value", what, f.val(limbs) / p)
        return
    inf = fm.is_zero_limbs(el[2])
    assert inf == (want is None), ("infinite: %s, the reference: %s" % (inf, want is None), what)
    if inf:
        return
    if y_bound == 3 and op.startswith("madd"):
        # the mixed addition's Y3 (ec.cuh ec_mulsub): one fused reduction over G1 (< 2p) and where the Fq2 product is inlined (BN254, and
        # the hot form everywhere: < 3p, BETA = 5: < 2p); two products and a sub<2> in the cold Fq2 kernels of the BLS curves (< 4p)
        fused = fm.group == 1 or op == "madd_hot" or fm.C.name == "bn128"
        y_bound = (2 if fm.group == 1 or f.beta != 1 else 3) if fused else 4
    bounds = (3, y_bound if kind == "plain" else 4, 2, 2) if fm.form == 1 else (1, 1, 1, 1)
    for s, (c, kp) in enumerate(zip(el, bounds)):
        for limbs in c:
            assert all(x <= fm.lo_max for x in limbs[:-1]), ("limb bound", s, what)
            assert f.val(limbs) < kp * p, ("value bound: %.3f p where < %d p is written" % (f.val(limbs) / p, kp), s, what)
    X, Y, ZZ, ZZZ = (fm.res(c) for c in el)
    assert not K.is_zero(ZZ) and not K.is_zero(ZZZ), ("a finite result with ZZ = 0 mod p", what)
    assert K.mul(K.mul(ZZ, ZZ), ZZ) == K.mul(ZZZ, ZZZ), ("ZZ^3 != ZZZ^2", what)
    assert X == K.mul(want[0], ZZ) and Y == K.mul(want[1], ZZZ), ("another point", what)


def run_op(ctx, fm, op):
    key = (fm.C.name, fm.group, fm.form, op)
    if key not in _cases:
        _cases[key] = build_cases(fm, op)
    A, Bs, flags, scal, sched, want, seen = _cases[key]
    kinds = OPS[op][5]
    # the reference's count of every kind: overall, in every run of 64 (the scheduled part), and the two uniform runs
    n = len(seen)
    uniform = 128 if OPS[op][3] and "dbl" in kinds else 0
    counts = {k: seen.count(k) for k in kinds}
    print("%s group %d form %d %s: %d elements, %s" % (fm.C.name, fm.group, fm.form, op, n, counts))
    assert set(seen) <= set(kinds), (set(seen) - set(kinds), "the operands left the function's precondition")
    assert all(counts[k] > 0 for k in kinds), counts
    assert seen == sched, [(i, s, w) for i, (s, w) in enumerate(zip(seen, sched)) if s != w][:5]
    for start in range(0, n - uniform, 64):
        assert set(seen[start:start + 64]) == set(kinds), (start, set(seen[start:start + 64]))
    if uniform:
        assert seen[n - 128:n - 64] == ["dbl"] * 64 and seen[n - 64:] == ["cancel"] * 64
    k = np.zeros((n, 8), dtype=np.uint32)
    for i, s in enumerate(scal):
        k[i] = [(s >> (32 * w)) & 0xffffffff for w in range(8)]
    a_arr, b_arr = to_array(fm, A), to_array(fm, Bs)
    got = ctx.group_op(fm.cid, fm.group, fm.form, op, a_arr, b_arr, k, np.array(flags, dtype=np.uint8))
    assert got.shape == a_arr.shape
    for i in range(n):
        try:
            check_element(fm, op, got[i], want[i], seen[i], (op, fm.C.name, fm.group, fm.form, i, seen[i]))
        except AssertionError as e:       # (the operands are only spelled out for the element that failed)
            hexed = lambda o: [[[hex(int(x)) for x in c] for c in coord] for coord in o]
            raise AssertionError("%s\nflags %d scalar %x\na = %r\nb = %r\ngot = %r" % (e, flags[i], scal[i], hexed(A[i]), hexed(Bs[i]), hexed(got[i])))


PARAMS = [(ci, group, form, op) for ci in range(3) for group in (1, 2) for form in (0, 1) for op, spec in OPS.items() if form in spec[0] and group in spec[1]]


@pytest.mark.parametrize("backend", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("ci,group,form,op", PARAMS, ids=["%s-g%d-f%d-%s" % (CURVES[ci][0].name, g, fo, op) for ci, g, fo, op in PARAMS])
def test_group_law(contexts, ci, group, form, op, backend):
    run_op(contexts(backend), form_of(ci, group, form), op)


@pytest.mark.parametrize("backend", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_unknown_ids_are_refused(contexts, backend):
    """every (group, form, op) outside the table is refused, as zkhip_field_op refuses fields above 5; the ids match native.GROUP_OPS"""
    ctx = contexts(backend)
    assert native.Context.GROUP_OPS == list(OPS)
    fm = form_of(0, 1, 1)
    z = np.zeros(4 * fm.f.N, dtype=np.uint32)
    k, fl = np.zeros(8, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
    out = np.zeros_like(z)
    call = lambda curve, group, form, op: ctx.lib.L.zkhip_group_op(ctx.h, curve, group, form, op, 1, native._ptr(z), native._ptr(z), native._ptr(k),
                                                                   native._ptr(fl), native._ptr(out))
    for group in (0, 1, 2, 3):
        for form in (-1, 0, 1, 2):
            for op in range(-1, len(OPS) + 2):
                name = list(OPS)[op] if 0 <= op < len(OPS) else None
                known = name is not None and form in OPS[name][0] and group in OPS[name][1]
                if not known:
                    assert call(0, group, form, op) != 0, (group, form, op)
    assert call(0, 1, 1, 7) == 0 and call(3, 1, 1, 7) != 0
