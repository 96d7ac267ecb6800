"""The written contracts of the unsaturated field (zokrates_amd/csrc/fieldu.cuh) at their edges, on every field.

tests/host/fieldu_contract.cpp is a thin driver: it puts the limbs it is given straight into Fu<P> / Fu2<P> objects, applies one
operation and prints the raw result.  Everything else is here, in Python big integers: the operands (built from each operation's
PRECONDITION: limbs at 2^B + 8, values within one of every multiple of p up to the stated bound, subtrahends at the bias's top
limb), the expected VALUE (sum of limb_i 2^(B i), congruent mod p; Montgomery products divide by R' = 2^(B N)) and the
POSTCONDITION the comment next to the operation states (limb bound, value bound, canonical).  CONTRACTS is that table.

A TIGHT spelling of a given integer is unique except at limbs whose low B bits are <= 8, so "several spellings of j p" exist only
where p's limbs allow: the "three spellings of every j p" the operand plan asks for cannot be had inside TIGHT.  respell generates
the spellings that move one unit from limb i + 1 into a limb i whose low bits are <= 8 (up to 15 subsets of such limbs); it does not
chain a borrow through a zero limb (i + 1 at 0 borrowing from i + 2), so those rarer spellings come only from the pattern operands,
which cover the redundant limbs (0, 1, 2^B - 1, 2^B, 2^B + 8 under every admissible top limb) without aiming at one integer."""
import os
import random
import subprocess

import pytest

import bls377_ref
from oracle.fields import BLS12_381, BN254

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zokrates_amd", "csrc")
SRC = os.path.join(HERE, "host", "fieldu_contract.cpp")


class Field:
    def __init__(self, name, p, B, N, fq, beta=1):
        self.name, self.p, self.B, self.N, self.fq, self.beta = name, p, B, N, fq, beta
        self.W = (p.bit_length() + 31) // 32
        self.R = 1 << (B * N)
        self.top_shift = B * (N - 1)
        self.loose = fq       # UConst::LOOSE_OK (the driver's "info" is checked against this)

    def split(self, x):       # the limbs of UConst::split: the top limb keeps every remaining bit
        m = (1 << self.B) - 1
        return [(x >> (self.B * i)) & m for i in range(self.N - 1)] + [x >> self.top_shift]

    def val(self, limbs):
        return sum(l << (self.B * i) for i, l in enumerate(limbs))

    def bias_top(self, K):    # top limb of UConst::bias(K) (the carried sub<K>) and of bias_spread(K, B + 1) (the lazy forms)
        return (K * self.p >> self.top_shift) - 4, (K * self.p >> self.top_shift) - 2


FIELDS = [
    Field("Bn254Fq", BN254.q, 29, 9, True), Field("Bls381Fq", BLS12_381.q, 28, 14, True), Field("Bls377Fq", bls377_ref.Q, 28, 14, True, beta=5),
    Field("Bn254Fr", BN254.r, 29, 9, False), Field("Bls381Fr", BLS12_381.r, 29, 9, False), Field("Bls377Fr", bls377_ref.R, 29, 9, False),
]

# ---------------------------------------------------------------- the contracts, as the comments state them
# Operand classes: ("T", k) a TIGHT element (every limb below the top one <= 2^B + 8) with value < k p;
#                  ("S", K) a TIGHT subtrahend of a carried sub<K>: value < K p and top limb <= (K p)_top - 2 (the carry round
#                           gives the top limb at least 2 of the 4 the bias holds back: any such b leaves it >= 0);
#                  ("L", K) the subtrahend of a lazy form: the same bound, there checked by ZK_LAZY_TOP_CHECK;
#                  ("C",)   a factor unpacked from its table: every limb below the top one < 2^B exactly, value < 2p;
#                  ("P",)   a TIGHT element with value < min(32p, 2^(32 W)): what fits the packed form;
#                  ("W",)   packed words, any value < 2^(32 W).
# Postcondition: (limb class, value bound in p or None, exact integer or None); "T" = TIGHT.
# op -> (operands, postcondition, where the contract is written).  Fq2 operations list their operands per component.
T8, T2 = ("T", 8), ("T", 2)
CONTRACTS = {
    "fe_add": ([("T", 16), ("T", 16)], ("T", 32, "a+b"), "fieldu.cuh:17 add: one carry round, TIGHT out"),
    "fe_dbl": ([("T", 16)], ("T", 32, "2a"), "fieldu.cuh:17"),
    "fe_sub_k2": ([("T", 16), ("S", 2)], ("T", 18, "a+2p-b"), "fieldu.cuh:17-21,227 sub<K>(a, b) = a + K p - b needs b < K p, top limb <= (K p)_top - 2"),
    "fe_sub_k4": ([("T", 16), ("S", 4)], ("T", 20, "a+4p-b"), "fieldu.cuh:227"),
    "fe_sub_k8": ([("T", 16), ("S", 8)], ("T", 24, "a+8p-b"), "fieldu.cuh:227"),
    "fe_sub_k16": ([("T", 16), ("S", 16)], ("T", 32, "a+16p-b"), "fieldu.cuh:227"),
    "fe_neg": ([("S", 2)], ("T", 2, "2p-a or 0"), "fieldu.cuh:237 value < 2p in, < 2p out, all-zero stays all-zero"),
    "fe_cneg": ([("S", 2)], ("T", 2, "2p-y | y"), "fieldu.cuh:289 normalised (TIGHT, < 2p)"),
    "fe_relax": ([("T", 32)], ("T", 3, None), "fieldu.cuh:464 TIGHT < 32p -> TIGHT < 3p"),
    "fe_is_zero_modp": ([("T", 32)], ("bool", None, None), "fieldu.cuh:486 x == 0 mod p for a TIGHT x < 32p"),
    "rp_canon": ([T2], ("canonical", 1, None), "kernels_ntt.cuh:46 TIGHT, value < 2p -> canonical packed words"),
    "fu_pack": ([("P",)], ("words", None, "a"), "fieldu.cuh:748 the integer value of a TIGHT element, < 2^(32W)"),
    "fu_unpack": ([("W",)], ("C", None, "a"), "fieldu.cuh:751 shifts and masks, the top limb keeps whatever is left"),
    "fu_mul_inl": ([T8, T8], ("T", 2, None), "fieldu.cuh:14 TIGHT operands < 8p, TIGHT result < 2p"),
    "fu_sqr_inl": ([T8], ("T", 2, None), "fieldu.cuh:14,415"),
    "fu_mul2_inl": ([T8] * 4, ("T", "sum2", None), "fieldu.cuh:15-16,433 base fields (R' >= 2^7 p): < 2p; see sum_bound"),
    "fu_mul4_inl": ([T8] * 8, ("T", "sum4", None), "fieldu.cuh:440 operand values < 8p: result < 3p for both base fields' R' >= 2^7 p"),
    "fu_mul_loose": ([T8, T8], ("T", 2, None), "fieldu.cuh:341-345,421 the same '< T / R' + p' as ever"),
    "fu_sqr_loose": ([T8], ("T", 2, None), "fieldu.cuh:421"),
    "fu_x3_numerator": ([T2, T2, T2], ("T", 10, "a+8p-b-2c"), "fieldu.cuh:303 operands TIGHT < 2p, result TIGHT < 10p"),
    "mul_neg_lazy": ([("L", 2), T8], ("T", 2, None), "fieldu.cuh:241-254 2p - a as one operand of a single product"),
    "mul_loose_neg_lazy": ([("L", 2), T8], ("T", 2, None), "fieldu.cuh:166-168,421 one lazily negated operand"),
    "mul2_neg_lazy": ([T8, T8, T8, ("L", 2)], ("T", 2, None), "fieldu.cuh:252 two-product sum, the other operands TIGHT; ec.cuh:69"),
    "mul2_loose_neg_lazy": ([T8, T8, T8, ("L", 2)], ("T", 2, None), "ec.cuh:69 the fused Y3 of the hot path"),
    "mul_cneg_for_mul": ([("L", 2), T8], ("T", 2, None), "fieldu.cuh:281 only feeds the product S2 = ZZZ1 * y; ec.cuh:214"),
    "mul2_cneg_for_mul": ([T8, T8, T8, ("L", 2)], ("T", 2, None), "fieldu.cuh:252,281"),
    "ntt_sub_lazy2": ([("T", 4), ("L", 2), ("C",)], ("T", 2, None), "fieldu.cuh:262-264 operand of one product against limbs < 2^B exactly"),
    "ntt_sub_lazy4": ([("T", 4), ("L", 4), ("C",)], ("T", 2, None), "kernels_ntt.cuh:470,495,508 differences < 12p, products < 2p"),
    "ntt_sub_lazy8": ([("T", 4), ("L", 8), ("C",)], ("T", 2, None), "kernels_ntt.cuh:506"),
    "ntt_add_lazy": ([("T", 6), ("T", 6), ("C",)], ("T", 2, None), "kernels_ntt.cuh:507 sums < 12p"),
    "ntt_first_round": ([("T", 3)] * 4 + [("C",)] * 4, ("T", 2, None), "kernels_ntt.cuh:470-474,533-552 inputs < 3p; products < 2p; the untwiddled output < 3p (fe_relax)"),
    "lds_ntt_dif4": ([("T", 3)] * 16 + [("C",)] * 13, ("T", 14, None), "kernels_ntt.cuh:470-474 a twiddled and the last round of 16 points: the last round leaves < 14p, its relaxed slot < 3p"),
    "lds_ntt_last4": ([("T", 3)] * 4 + [("C",)], ("T", 14, None), "kernels_ntt.cuh:470-474,509-512 the untwiddled round on inputs < 3p: < 14p, its relaxed slot < 3p"),
    "ec_inv": ([("T", 8)], ("T", 2, None), "fieldu.cuh:685 x TIGHT < 8p, non-zero mod p; the result is TIGHT, < 2p"),
}
# Fq2: (a0, a1[, b0, b1 ...]); the second factor's c1 is negated as 8p - b1 without a carry round ("L", 8)
CONTRACTS_FQ2 = {
    "ec_mul2x": ([T8, T8, T8, ("L", 8)], ("T", 2, None), "fieldu.cuh:579-585 results that stay below 2p whatever the operands"),
    "fu2_mul_loose": ([T8, T8, T8, ("L", 8)], ("T", 2, None), "fieldu.cuh:582, kernels_msm's hot path"),
    "ec_sqr2x": ([("T", 6), ("L6", 8)], ("T", 2, None), "fieldu.cuh:595 operands < 6p: result below 2p"),
    "fu2_sqr_loose": ([("T", 6), ("L6", 8)], ("T", 2, None), "fieldu.cuh:595-609"),
    "fu2_mulsub_loose": ([T8, T8, T8, ("L", 8), T8, T8, ("S", 8), ("S", 8)], ("T", 3, None), "fieldu.cuh:440,562,664 a component < 3p (BETA = 5: < 2p)"),
    "fu2_mul_kara": ([("T", 4), ("T", 4), T2, T2], ("T", 2, None), "fieldu.cuh:615 a < 4p per component, b < 2p per component"),
    "ec_inv2x": ([T8, ("S", 8)], ("T", 2, None), "fieldu.cuh:792 products of TIGHT operands: < 2p"),
}
LOOSE_ONLY = {"fu_mul_loose", "fu_sqr_loose", "mul_loose_neg_lazy", "mul2_loose_neg_lazy"}       # where UConst<P>::LOOSE_OK


# ---------------------------------------------------------------- operands
def limit_of(f, cls):
    """(value bound, top-limb cap or None, lower-limb maximum) of an operand class"""
    kind = cls[0]
    if kind == "T":
        return cls[1] * f.p, None, (1 << f.B) + 8
    if kind == "S" or kind == "L":
        return cls[1] * f.p, f.bias_top(cls[1])[1], (1 << f.B) + 8
    if kind == "L6":     # the squared element's c1: < 6p, and negated against the spread 8p
        return 6 * f.p, f.bias_top(cls[1])[1], (1 << f.B) + 8
    if kind == "C":
        return 2 * f.p, None, (1 << f.B) - 1
    if kind == "P":      # anything TIGHT that fits the packed words
        return min(32 * f.p, 1 << (32 * f.W)), None, (1 << f.B) + 8
    raise AssertionError(cls)


def admissible(f, cls, limbs):
    bound, top_cap, lo_max = limit_of(f, cls)
    return (all(0 <= l <= lo_max for l in limbs[:-1]) and 0 <= limbs[-1] < (1 << 32) and f.val(limbs) < bound
            and (top_cap is None or limbs[-1] <= top_cap))


def respell(f, limbs, lo_max, rnd):
    """every other TIGHT spelling of the same integer: a limb whose low bits are small may take 2^B from the limb above"""
    out = []
    spots = [i for i in range(f.N - 1) if limbs[i] + (1 << f.B) <= lo_max and limbs[i + 1] >= 1]
    for mask in range(1, min(1 << len(spots), 16)):
        l = list(limbs)
        ok = True
        for k, i in enumerate(spots):
            if mask >> k & 1:
                if l[i + 1] < 1 or l[i] + (1 << f.B) > lo_max:
                    ok = False
                    break
                l[i] += 1 << f.B
                l[i + 1] -= 1
        if ok and all(x >= 0 for x in l):
            out.append(l)
    return out


def boundary_operands(f, cls, rnd, n_pattern=40):
    """Operands built from the precondition `cls` (see CONTRACTS): exact values at the edges in every spelling, and limb patterns
    from {0, 1, 2^B - 1, 2^B, 2^B + 8} under a top limb that puts the value at 0, at the largest admissible one, and next to
    every multiple of p inside the range."""
    bound, top_cap, lo_max = limit_of(f, cls)
    B, N, p = f.B, f.N, f.p
    kmax = bound // p
    vals = {0, 1, 2, bound - 1, bound - 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, f.R % p, (f.R % p) - 1, (1 << (32 * f.W)) % p}
    for j in range(1, kmax + 1):
        vals.update((j * p - 1, j * p, j * p + 1))
    for k in list(range(B - 1, B * N, B)) + list(range(B, B * N, B)) + list(range(32, 32 * f.W, 32)):
        vals.update(((1 << k) - 1, 1 << k, (1 << k) + 1))
    if top_cap is not None:       # a top limb exactly at the bias's, everything below it as large as it may be
        vals.add(min(bound - 1, ((top_cap + 1) << f.top_shift) - 1))
        vals.add(top_cap << f.top_shift)
    out = []
    for v in sorted(vals):
        if not 0 <= v < bound:
            continue
        l = f.split(v)
        out.append(l)
        out += respell(f, l, lo_max, rnd)
    S = [0, 1, (1 << B) - 1, 1 << B, (1 << B) + 8] if lo_max > (1 << B) else [0, 1, (1 << B) - 2, (1 << B) - 1]
    patterns = [[s] * (N - 1) for s in S] + [[rnd.choice(S) for _ in range(N - 1)] for _ in range(n_pattern)]
    for lo in patterns:
        lv = sum(x << (B * i) for i, x in enumerate(lo))
        tops = {0}
        if bound - 1 >= lv:
            tops.add((bound - 1 - lv) >> f.top_shift)
        for j in range(1, kmax + 1):
            t = (j * p - lv) >> f.top_shift
            tops.update((t - 1, t, t + 1))
        if top_cap is not None:
            tops.add(top_cap)
        for t in tops:
            out.append(lo + [t])
    return [l for l in out if admissible(f, cls, l)]


def random_operand(f, cls, rnd):
    bound, top_cap, lo_max = limit_of(f, cls)
    while True:
        mode = rnd.randrange(3)
        if mode == 0:      # a uniform value, canonical limbs
            l = f.split(rnd.randrange(bound))
        elif mode == 1:    # uniform redundant limbs under a uniform top limb
            l = [rnd.randrange(lo_max + 1) for _ in range(f.N - 1)] + [rnd.randrange((bound >> f.top_shift) + 1)]
        else:              # what a carry round leaves: low bits plus a small carry
            l = f.split(rnd.randrange(bound))
            l = [min(lo_max, x + rnd.randrange(7)) if i and i < f.N - 1 else x for i, x in enumerate(l)]
        if admissible(f, cls, l):
            return l


def cases_for(f, classes, seed, n_boundary=260, n_random=260):
    """Operand tuples for one operation: every operand in turn walks its boundary list while the others take boundary or random
    values; then seeded random tuples."""
    rnd = random.Random(seed)
    pools = [boundary_operands(f, c, rnd) for c in classes]
    cases = []
    per = max(1, n_boundary // len(classes))
    for k, pool in enumerate(pools):
        picks = pool if len(pool) <= per else [pool[0], pool[-1]] + rnd.sample(pool, per - 2)
        for x in picks:
            cases.append([x if i == k else (rnd.choice(pools[i]) if rnd.random() < 0.6 else random_operand(f, classes[i], rnd)) for i in range(len(classes))])
    # every operand at its largest value together, and at zero together
    big = [max(pl, key=f.val) for pl in pools]
    cases.append(big)
    cases.append([min(pl, key=f.val) for pl in pools])
    # the same element in every slot (a - a, a * a) where the classes allow it
    for x in pools[0][:: max(1, len(pools[0]) // 12)]:
        if all(admissible(f, c, x) for c in classes):
            cases.append([x] * len(classes))
    for _ in range(n_random):
        cases.append([random_operand(f, c, rnd) for c in classes])
    return cases


# ---------------------------------------------------------------- the driver
def build_driver(tmp, sanitize):
    exe = os.path.join(tmp, "fieldu_contract" + ("_san" if sanitize else ""))
    cmd = ["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-DZK_CHECK_OVERFLOW"] + (["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"] if sanitize else [])
    subprocess.check_call(cmd + ["-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("fieldu_contract")), request.param)


def run_driver(exe, lines):
    return subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)


def line_of(f, op, operands):
    return "%s %s %s" % (f.name, op, " ".join("%x" % w for l in operands for w in l))


# ---------------------------------------------------------------- expected values and postconditions
def sum_bound(f, nt):
    """A sum of nt products of operands < 8p, reduced once: (nt * 64 p^2) / R' + p.  The comments state it for the base fields, whose
    R' >= 2^7 p: < 2p for two products, < 3p for four.  A scalar field of 255 bits has R' >= 2^6 p only: < 3p and < 5p there (no
    caller sums products over a scalar field; the bound is the same formula)."""
    return -(-nt * 64 * f.p // f.R) + 1


def check_post(f, post, limbs, what):
    kind, kp, _ = post
    if kp in ("sum2", "sum4"):
        stated = 2 if kp == "sum2" else 3
        kp = sum_bound(f, int(kp[3]))
        if f.fq:
            assert kp <= stated      # the formula gives what the comment states
            kp = stated
    assert len(limbs) == f.N, what
    lo_max = (1 << f.B) + 8 if kind == "T" else (1 << f.B) - 1
    assert all(l <= lo_max for l in limbs[:-1]), ("limb bound", what, [hex(x) for x in limbs])
    if kp is not None:
        v = f.val(limbs)
        assert v < kp * f.p, ("value bound: %.3f p where < %d p is promised" % (v / f.p, kp), what)


def expected_fu(f, op, a):
    """(value mod p, exact integer or None) from the operands' integer values"""
    p, R = f.p, f.R
    Rinv = pow(R, -1, p)
    v = [f.val(x) for x in a]
    if op == "fe_add": return None, v[0] + v[1]
    if op == "fe_dbl": return None, 2 * v[0]
    if op.startswith("fe_sub_k"):
        K = int(op[8:])
        return None, v[0] + K * p - v[1]
    if op == "fu_x3_numerator": return None, v[0] + 8 * p - v[1] - 2 * v[2]
    if op in ("fu_mul_inl", "fu_mul_loose"): return v[0] * v[1] * Rinv % p, None
    if op in ("fu_sqr_inl", "fu_sqr_loose"): return v[0] * v[0] * Rinv % p, None
    if op == "fu_mul2_inl": return (v[0] * v[1] + v[2] * v[3]) * Rinv % p, None
    if op == "fu_mul4_inl": return (v[0] * v[1] + v[2] * v[3] + v[4] * v[5] + v[6] * v[7]) * Rinv % p, None
    if op in ("mul_neg_lazy", "mul_loose_neg_lazy"): return -v[0] * v[1] * Rinv % p, None
    if op in ("mul2_neg_lazy", "mul2_loose_neg_lazy", "mul2_cneg_for_mul"): return (v[0] * v[1] - v[2] * v[3]) * Rinv % p, None
    if op.startswith("ntt_sub_lazy"): return (v[0] - v[1]) * v[2] * Rinv % p, None
    if op == "ntt_add_lazy": return (v[0] + v[1]) * v[2] * Rinv % p, None
    if op == "fe_relax": return v[0] % p, None
    if op == "ec_inv": return pow(v[0] * Rinv % p, -1, p) * R % p, None      # x^(p-2) in Montgomery form: R'^2 / x
    raise AssertionError(op)


def judge(f, op, operands, words):
    """the driver's answer to one case against value and postcondition"""
    classes, post, _ = (CONTRACTS_FQ2 if op in CONTRACTS_FQ2 else CONTRACTS)[op]
    p, N = f.p, f.N
    what = (f.name, op, [[hex(x) for x in l] for l in operands])
    v = [f.val(x) for x in operands]
    if op == "fe_is_zero_modp":
        assert words == [1 if v[0] % p == 0 else 0], what
    elif op == "rp_canon":
        got = sum(w << (32 * i) for i, w in enumerate(words))
        assert len(words) == f.W and got == v[0] % p, ("canonical", what, hex(got))
    elif op == "fu_pack":
        assert len(words) == f.W and sum(w << (32 * i) for i, w in enumerate(words)) == v[0], what
    elif op == "fu_unpack":
        x = sum(w << (32 * i) for i, w in enumerate(operands[0]))
        limbs, again = words[:N], words[N:]
        assert all(l < (1 << f.B) for l in limbs[:-1]) and f.val(limbs) == x and again == list(operands[0]), what
    elif op == "fe_neg":
        if all(x == 0 for x in operands[0]):
            assert words == [0] * N, what
        else:
            check_post(f, ("T", None, None), words, what)
            assert f.val(words) == 2 * p - v[0], what
            assert f.val(words) < 2 * p or v[0] == 0, what
    elif op == "fe_cneg":
        neg, same = words[:N], words[N:]
        check_post(f, post, neg, what) if v[0] > 0 else check_post(f, ("T", None, None), neg, what)
        check_post(f, post, same, what)
        assert f.val(neg) == 2 * p - v[0] and f.val(same) == v[0], what
    elif op == "mul_cneg_for_mul":
        Rinv = pow(f.R, -1, p)
        neg, same = words[:N], words[N:]
        check_post(f, post, neg, what)
        check_post(f, post, same, what)
        assert f.val(neg) % p == -v[0] * v[1] * Rinv % p and f.val(same) % p == v[0] * v[1] * Rinv % p, what
    elif op == "ntt_first_round":
        # (a, b, c, d) -> a + b + c + d | (a - b + c - d) w^2pos | (a - c + w4 (b - d)) w^pos | (a - c - w4 (b - d)) w^3pos
        Rinv = pow(f.R, -1, p)
        xa, xb, xc, xd, w1, w2, w3, w4 = v
        t3 = (xb - xd) * w4 * Rinv
        want = [xa + xb + xc + xd, (xa - xb + xc - xd) * w2 * Rinv, (xa - xc + t3) * w1 * Rinv, (xa - xc - t3) * w3 * Rinv]
        for k in range(4):
            limbs = words[k * N:(k + 1) * N]
            check_post(f, ("T", 3 if k == 0 else 2, None), limbs, what + (k,))
            assert f.val(limbs) % p == want[k] % p, ("value", what, k)
    elif op == "lds_ntt_last4":
        Rinv = pow(f.R, -1, p)
        xa, xb, xc, xd, w4 = v
        t3 = (xb - xd) * w4 * Rinv
        want = [xa + xb + xc + xd, xa - xb + xc - xd, xa - xc + t3, xa - xc - t3]
        for k in range(4):
            limbs = words[k * N:(k + 1) * N]
            check_post(f, ("T", 3 if k == 0 else 14, None), limbs, what + (k,))
            assert f.val(limbs) % p == want[k] % p, ("value", what, k)
    elif op == "lds_ntt_dif4":
        # the network of lds_ntt_dif4 for 16 points over the plan's 13 factors: round L = 16 (butterfly pos = 0 .. 3 on slots pos + 4 k,
        # factors plan[pos], plan[4 + pos], plan[8 + pos]), then round L = 4 (slots 4 g + k, no factor but w4 = plan[12])
        Rinv = pow(f.R, -1, p)
        x, plan = list(v[:16]), v[16:]
        w4 = plan[12]

        def butterfly(idx, f1, f2, f3):
            xa, xb, xc, xd = (x[i] for i in idx)
            t3 = (xb - xd) * w4 * Rinv
            outs = [xa + xb + xc + xd, (xa - xb + xc - xd) * f2, (xa - xc + t3) * f1, (xa - xc - t3) * f3]
            for i, y in zip(idx, outs):
                x[i] = y % p
        for pos in range(4):
            butterfly([pos, pos + 4, pos + 8, pos + 12], plan[pos] * Rinv, plan[4 + pos] * Rinv, plan[8 + pos] * Rinv)
        for g in range(4):
            butterfly([4 * g, 4 * g + 1, 4 * g + 2, 4 * g + 3], 1, 1, 1)
        for k in range(16):
            limbs = words[k * N:(k + 1) * N]
            check_post(f, ("T", 3 if k % 4 == 0 else 14, None), limbs, what + (k,))
            assert f.val(limbs) % p == x[k], ("value", what, k)
    elif op in CONTRACTS_FQ2:
        Rinv = pow(f.R, -1, p)
        m = [x * Rinv % p for x in v]       # the plain residues
        F2 = bls377_ref.Fq2Beta(p, f.beta)
        el = [(m[i], m[i + 1]) for i in range(0, len(m), 2)]
        if op in ("ec_mul2x", "fu2_mul_loose", "fu2_mul_kara"): want = F2.mul(el[0], el[1])
        elif op in ("ec_sqr2x", "fu2_sqr_loose"): want = F2.mul(el[0], el[0])
        elif op == "fu2_mulsub_loose": want = F2.sub(F2.mul(el[0], el[1]), F2.mul(el[2], el[3]))
        else: want = F2.inv(el[0])
        kp = 2 if (op == "fu2_mulsub_loose" and f.beta != 1) else post[1]
        for c, limbs in enumerate((words[:N], words[N:])):
            check_post(f, ("T", kp, None), limbs, what + (c,))
            assert f.val(limbs) % p == want[c] * f.R % p, ("value", what, c)
    else:
        check_post(f, post, words, what)
        modp, exact = expected_fu(f, op, operands)
        if exact is not None:
            assert f.val(words) == exact, ("exact value", what, [hex(x) for x in words])
        else:
            assert f.val(words) % p == modp, ("value", what, [hex(x) for x in words])


def ops_of(f):
    ops = [op for op in CONTRACTS if (f.loose or op not in LOOSE_ONLY) and (f.N <= 12 or op not in ("ntt_first_round", "lds_ntt_dif4", "lds_ntt_last4"))]      # (a plan entry holds 12 limbs)
    return ops + (list(CONTRACTS_FQ2) if f.fq else [])


def operands_for(f, op):
    seed = "%s/%s" % (f.name, op)
    if op == "fu_unpack":
        rnd = random.Random(seed)
        top = 1 << (32 * f.W)
        vals = [0, 1, top - 1, top - 2, f.p, f.p - 1, 2 * f.p - 1, f.R % f.p] + [(1 << k) + d for k in range(f.B - 1, 32 * f.W, f.B) for d in (-1, 0)]
        vals += [(1 << k) - 1 for k in range(32, 32 * f.W, 32)] + [rnd.randrange(top) for _ in range(300)]
        return [[[(x >> (32 * i)) & 0xffffffff for i in range(f.W)]] for x in vals if 0 <= x < top]
    if op in CONTRACTS_FQ2:
        classes = CONTRACTS_FQ2[op][0]
        cases = cases_for(f, classes, seed, n_boundary=200, n_random=200)
        if op == "ec_inv2x":      # not the zero element
            cases = [c for c in cases if any(f.val(x) % f.p for x in c)]
            cases = cases[:: max(1, len(cases) // 40)]          # (an inversion is 600 products)
        return cases
    classes = CONTRACTS[op][0]
    if op in ("fe_relax", "fe_is_zero_modp"):
        # every j p, j = 0 ... 31, in each spelling there is, and j p +- 1; then the general classes
        rnd = random.Random(seed)
        extra = []
        for j in range(32):
            for d in (-1, 0, 1):
                x = j * f.p + d
                if x >= 0:
                    l = f.split(x)
                    extra += [[l]] + [[s] for s in respell(f, l, (1 << f.B) + 8, rnd)]
                    # the multiple itself under limbs a carry round leaves (one unit moved down from limb i + 1 where it fits)
                    for i in range(f.N - 1):
                        if l[i + 1] >= 1 and l[i] + (1 << f.B) <= (1 << f.B) + 8:
                            m = list(l); m[i] += 1 << f.B; m[i + 1] -= 1
                            extra.append([m])
        return extra + cases_for(f, classes, seed)
    if op == "ec_inv":
        cases = [c for c in cases_for(f, classes, seed) if f.val(c[0]) % f.p]
        return cases[:: max(1, len(cases) // 60)]
    return cases_for(f, classes, seed)


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_contracts(driver, f):
    """Every operation of the table on this field: value and postcondition of every case, the program exits 0 (no column left 64
    bits, no lazy top limb above its bias), and the driver's own count says every (field, op) pair ran."""
    info = run_driver(driver, ["%s info" % f.name])
    assert info.returncode == 0, info.stderr
    assert [int(x, 16) for x in info.stdout.splitlines()[0].split()] == [f.B, f.N, f.W, 1 if f.loose else 0]
    ops = ops_of(f)
    lines, todo = [], []
    for op in ops:
        for operands in operands_for(f, op):
            lines.append(line_of(f, op, operands))
            todo.append((op, operands))
    out = run_driver(driver, lines)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = out.stdout.splitlines()
    results = [r for r in rows if not r.startswith("count ")]
    counts = {r.split()[2]: int(r.split()[3]) for r in rows if r.startswith("count ")}
    assert len(results) == len(todo)
    for op in ops:
        n = counts.get(op, 0)
        print("%s %s: %d cases" % (f.name, op, n))
        assert n > 0 and n == sum(1 for o, _ in todo if o == op), (f.name, op)
        assert n >= (20 if op.startswith("ec_inv") else 200), (f.name, op, n)
    for (op, operands), row in zip(todo, results):
        judge(f, op, operands, [int(x, 16) for x in row.split()])


def _neg_controls(f):
    """one operand per guarded precondition that breaks it by the least amount"""
    B, N = f.B, f.N
    tight = f.split(f.p - 1)
    unit = [1] + [0] * (N - 1)
    out = []
    for op, K, slot, arity in (("mul_neg_lazy", 2, 0, 2), ("mul_cneg_for_mul", 2, 0, 2), ("mul2_neg_lazy", 2, 3, 4), ("ntt_sub_lazy2", 2, 1, 3),
                               ("ntt_sub_lazy4", 4, 1, 3), ("ntt_sub_lazy8", 8, 1, 3)):
        bad = [0] * (N - 1) + [f.bias_top(K)[1] + 1]                 # a top limb one above the spread bias's
        out.append((op, [bad if i == slot else (unit if op.startswith("ntt") and i == 2 else tight) for i in range(arity)], "top limb"))
    # the carried sub<K> and fe_cneg: a subtrahend with the top limb of K p over a full limb below it leaves the result's top limb negative
    for op, K in (("fe_sub_k2", 2), ("fe_sub_k4", 4), ("fe_sub_k8", 8), ("fe_sub_k16", 16)):
        out.append((op, [[0] * N, [0] * (N - 2) + [(1 << B) + 8, K * f.p >> f.top_shift]], "the top limb wraps"))
    out.append(("fe_cneg", [[0] * (N - 2) + [(1 << B) + 8, 2 * f.p >> f.top_shift]], "the top limb wraps"))
    # a column that leaves 64 bits: every limb of both factors at 2^32 - 1
    full = [0xffffffff] * N
    out.append(("fu_mul_inl", [full, full], "overflows 64 bits"))
    out.append(("fu_mul4_inl", [full] * 8, "overflows 64 bits"))
    if f.fq:
        bad = [0] * (N - 1) + [f.bias_top(8)[1] + 1]
        out.append(("ec_mul2x", [tight, tight, tight, bad], "top limb"))
    return out


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_negative_controls_abort(driver, f):
    """The checks that make `exit 0` mean something are alive on this field: an operand one above a guarded precondition aborts the
    program with the check's message, and the same case one step inside the precondition runs."""
    for op, operands, message in _neg_controls(f):
        out = run_driver(driver, [line_of(f, op, operands)])
        assert out.returncode not in (0, 3) and message in out.stderr, (f.name, op, out.returncode, out.stderr[-500:])
        if message == "top limb":
            inside = [list(l) for l in operands]
            for l in inside:
                if l[:-1] == [0] * (f.N - 1) and l[-1] > 1:
                    l[-1] -= 1
            ok = run_driver(driver, [line_of(f, op, inside)])
            assert ok.returncode == 0, (f.name, op, ok.stderr[-500:])


def test_table_is_complete():
    """every operation the driver knows has a contract here, and the other way round"""
    src = open(SRC).read()
    import re
    known = set(re.findall(r'op == "([a-z0-9_]+)"', src)) - {"info"}
    assert known == set(CONTRACTS) | set(CONTRACTS_FQ2)
