"""The pairing check on the device (zokrates_amd/csrc/pairing.cuh): the Fq12 arithmetic one function at a time and the primitive
zkhip_pairing_products, against oracle/pairing.py's flat degree-12 field and its affine Miller loop.  One body: on the emulator
build in the CPU suite, on the GPU under `-m gpu`; three curves.

Tower ops (zkhip_tower_op, raw limbs in the kernel's own layout).  Operands: 65 seeded random elements; elements whose twelve
Fq coefficients are all 0, all 1, all p - 1; and the top of the stated operand range — every limb below the top one at 2^B + 8
and the value the largest below 3p that spelling allows, in all twelve coefficients.  Random elements are spelled as x R' + j p,
j = 0, 1, 2 by turns (the bound is 3p), canonical limbs.  Checked on every result, exactly: the residue is the oracle's; every limb
below the top one <= 2^B + 8; the value < 3p (the bound the kernel keeps for what it stores).  Identities, device against device:
inverse times value = 1; conj6 is the sixth power of the Frobenius map, and its twelfth power is the identity (the map has
order 12 on Fq12: six applications give w -> -w, not the identity).

The primitive.  G = native PAIR_ITEMS = 8 is the number of items one wavefront carries; a workgroup is one wavefront, so the
counts around G are the counts around a workgroup's load too, and 2G + 1 adds a third workgroup with one item.  Truth comes from
the oracle's pairing_product_is_one for the distinct items (slow: a second or two each, computed once per curve and shared by
both backends) and from bilinearity — e(aP, bQ) e(-abP, Q) = 1 and, with ab + 1, != 1 — where only the count matters.

The host verifier as the truth.  tests/host/device_verify.cpp (its own `main`, the compiled host layer, the emulator library)
holds Hip::verify_batch and zkhip_verify_*_batch to the host `verify` over ONE batch with the whole mutation set — good proofs,
one made with every blinding scalar 0, A, B, C negated, an input changed, two items' inputs swapped, a Groth16 proof whose A the
prover itself left at infinity (a key rewritten as in tests/test_degenerate_bases.py), and all of them under another setup's key
— and zkhip_pairing_products to the host's pairing_product_is_one; it also hands Hip::verify_batch a proof of another curve.

Left to the device alone, and why: the emulator half of the mutation test takes bn128 only (a dozen batches of two workgroups
are a minute per BLS curve there; the GPU half takes all three curves), and the input counts 0, 1 and 65 are run on bn128 (both
schemes): the input combination is the same kernel over each curve's own saturated field, which every curve's l = 5 case runs.
No sanitizer build of the program is made."""
import json
import os
import random

import numpy as np
import pytest

import bls377_ref
from oracle import pairing
from oracle.curves import groups
from oracle.fields import BLS12_381, BN254
from test_group_law import nth_root
from zokrates_amd import native

from emu_util import emu_library

CURVES = [(BN254, 0, 29, 9), (BLS12_381, 1, 28, 14), (bls377_ref.CURVE, 2, 28, 14)]      # curve, id, bits per limb, limbs
G = 8                      # items one wavefront (= one workgroup) carries: csrc/pairing.cuh PAIR_ITEMS
BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
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


def groups_of(curve):
    return bls377_ref.groups377(curve) if curve.name == "bls12_377" else groups(curve)


# ---------------------------------------------------------------- limbs
class Limbs:
    def __init__(self, curve, bits, n):
        self.p, self.B, self.N = curve.q, bits, n
        self.R = pow(2, bits * n, self.p)
        self.Rinv = pow(self.R, -1, self.p)
        fat = sum(((1 << bits) + 8) << (bits * i) for i in range(n - 1))
        top = (3 * self.p - 1 - fat) >> (bits * (n - 1))
        self.edge = ([(1 << bits) + 8] * (n - 1) + [top], (fat + (top << (bits * (n - 1)))) * self.Rinv % self.p)   # (limbs, the value they stand for)

    def enc(self, v, j=0):
        m = v * self.R % self.p + j * self.p
        mask = (1 << self.B) - 1
        return [(m >> (self.B * i)) & mask for i in range(self.N - 1)] + [m >> (self.B * (self.N - 1))]

    def dec(self, limbs):
        m = sum(int(l) << (self.B * i) for i, l in enumerate(limbs))
        assert all(int(l) <= (1 << self.B) + 8 for l in limbs[:-1]), "a limb above 2^B + 8"
        assert m < 3 * self.p, "a value of %.3f p" % (m / self.p)
        return m * self.Rinv % self.p


def to_flat(ctx, coefs):
    """six Fq2 coefficients of w^0 .. w^5 -> the oracle's flat element"""
    r = ctx.zero()
    for i, c in enumerate(coefs):
        r = ctx.add(r, ctx.mul(ctx.from_fq2(c), ctx.w_pow(i)))
    return r


def from_flat(ctx, f):
    return [((f[i] + ctx.xi0 * f[i + 6]) % ctx.q, f[i + 6] % ctx.q) for i in range(6)]


def line_positions(ctx):
    return (0, 1, 3) if ctx.twist_d else (0, 2, 3)


_tower_cases = {}


def tower_cases(ci):
    """(a, b) operand lists as (coefficients, spelling j or "edge") and the oracle's results per op, once per curve"""
    if ci in _tower_cases:
        return _tower_cases[ci]
    curve = CURVES[ci][0]
    ctx = pairing.Fq12Ctx(curve)
    rnd = random.Random(0x70e12 + ci)
    p = curve.q
    el = lambda: [(rnd.randrange(p), rnd.randrange(p)) for _ in range(6)]
    const = lambda v: [(v, v)] * 6
    A = [(el(), k % 3) for k in range(65)] + [(const(0), 0), (const(1), 0), (const(p - 1), 0), (const(1), 2), (None, "edge")]
    Bv = [(el(), (k + 1) % 3) for k in range(65)] + [(const(p - 1), 0), (const(0), 0), (const(1), 1), (None, "edge"), (None, "edge")]
    _tower_cases[ci] = (ctx, A, Bv)
    return _tower_cases[ci]


def spell(L, operands):
    out = np.zeros((len(operands), 6, 2, L.N), dtype=np.uint32)
    vals = []
    for n, (coefs, j) in enumerate(operands):
        if j == "edge":
            coefs = [(L.edge[1], L.edge[1])] * 6
        for i in range(6):
            for c in range(2):
                out[n, i, c] = L.edge[0] if j == "edge" else L.enc(coefs[i][c], j)
        vals.append(coefs)
    return out, vals


def read(L, raw):
    return [[(L.dec(raw[n, i, 0]), L.dec(raw[n, i, 1])) for i in range(6)] for n in range(raw.shape[0])]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ci", range(3), ids=[c[0].name for c in CURVES])
def test_tower_ops(contexts, ci, backend):
    curve, cid, bits, n = CURVES[ci]
    L = Limbs(curve, bits, n)
    ctx, A, Bv = tower_cases(ci)
    dev = contexts(backend)
    a_raw, a_val = spell(L, A)
    b_raw, b_val = spell(L, Bv)
    fa = [to_flat(ctx, v) for v in a_val]
    fb = [to_flat(ctx, v) for v in b_val]
    pos = line_positions(ctx)
    want = {
        "mul": [ctx.mul(x, y) for x, y in zip(fa, fb)],
        "sqr": [ctx.mul(x, x) for x in fa],
        "mul_line": [ctx.mul(x, to_flat(ctx, [v[i] if i in pos else (0, 0) for i in range(6)])) for x, v in zip(fa, b_val)],
        "inv": [ctx.inv(x) if any(x) else ctx.zero() for x in fa],
        "frobenius": [ctx.pow(x, curve.q) for x in fa],
        "conj6": [to_flat(ctx, [c if i % 2 == 0 else ((-c[0]) % curve.q, (-c[1]) % curve.q) for i, c in enumerate(v)]) for v in a_val],
    }
    got_raw = {}
    for op in native.Context.TOWER_OPS:
        got_raw[op] = dev.tower_op(cid, op, a_raw, b_raw)
        got = read(L, got_raw[op])
        for k in range(len(A)):
            assert got[k] == from_flat(ctx, want[op][k]), (curve.name, op, k)
    # identities, device against device
    one = from_flat(ctx, ctx.one())
    prod = read(L, dev.tower_op(cid, "mul", got_raw["inv"], a_raw))
    for k in range(len(A)):
        assert prod[k] == (one if any(fa[k]) else from_flat(ctx, ctx.zero())), (curve.name, "inverse times value", k)
    f = a_raw
    for times in range(1, 13):
        f = dev.tower_op(cid, "frobenius", f, b_raw)
        if times == 6:
            assert read(L, f) == read(L, got_raw["conj6"]), (curve.name, "Frobenius^6 = conj6")
    assert read(L, f) == [[(c[0] % curve.q, c[1] % curve.q) for c in v] for v in a_val], (curve.name, "Frobenius^12 = identity")


# ---------------------------------------------------------------- the primitive
def rec1(P, nb):
    return bytes(2 * nb) + b"\x01" if P is None else int(P[0]).to_bytes(nb, "little") + int(P[1]).to_bytes(nb, "little") + b"\x00"


def rec2(Q, nb):
    if Q is None:
        return bytes(4 * nb) + b"\x01"
    return b"".join(int(v).to_bytes(nb, "little") for v in (Q[0][0], Q[0][1], Q[1][0], Q[1][1])) + b"\x00"


def run_items(dev, curve, cid, items):
    """items: lists of (P, Q) of one length -> the device's verdicts"""
    nb = curve.fq_bytes
    g1 = b"".join(rec1(P, nb) for it in items for P, _ in it)
    g2 = b"".join(rec2(Q, nb) for it in items for _, Q in it)
    return list(dev.pairing_products(cid, len(items[0]), np.frombuffer(g1, dtype=np.uint8), np.frombuffer(g2, dtype=np.uint8)))


def fq2_sqrt(a, q, beta):
    """a square root in Fq[u] / (u^2 + beta), or None"""
    a0, a1 = a[0] % q, a[1] % q
    half = pow(2, -1, q)
    if a1 == 0:
        r = nth_root(a0, 2, q)
        if r is not None and r * r % q == a0:
            return (r, 0)
        r = nth_root(a0 * pow(-beta, -1, q) % q, 2, q)
        return None if r is None or (-beta * r * r) % q != a0 else (0, r)
    s = nth_root((a0 * a0 + beta * a1 * a1) % q, 2, q)
    if s is None or s * s % q != (a0 * a0 + beta * a1 * a1) % q:
        return None
    for sg in (s, -s):
        x0 = nth_root((a0 + sg) * half % q, 2, q)
        if x0 is not None and x0 and x0 * x0 % q == (a0 + sg) * half % q:
            x1 = a1 * pow(2 * x0, -1, q) % q
            if ((x0 * x0 - beta * x1 * x1) % q, 2 * x0 * x1 % q) == (a0, a1):
                return (x0, x1)
    return None


def off_subgroup(curve, group, which):
    """a point on the curve (which = 1) or the twist (2) whose order is not r"""
    q = curve.q
    x = 1
    while True:
        if which == 1:
            y = nth_root((x * x * x + group.b) % q, 2, q)
            P = None if y is None else (x, y)
        else:
            beta = 5 if curve.name == "bls12_377" else 1
            F = group.F
            X = (x, 1)
            y = fq2_sqrt(F.add(F.mul(F.mul(X, X), X), group.b), q, beta)
            P = None if y is None else (X, y)
        if P is not None and group.on_curve(P) and group.amul(P, curve.r) is not None:
            return P
        x += 1


_primitive = {}


def primitive_cases(ci):
    """[(name, pairs, verdict)] with the oracle's verdicts for the items whose points are admitted and 0 for the others, once per curve"""
    if ci in _primitive:
        return _primitive[ci]
    curve = CURVES[ci][0]
    G1, G2 = groups_of(curve)
    ctx = pairing.Fq12Ctx(curve)
    rnd = random.Random(0x9a1 + ci)
    r = curve.r
    a, b, c, d = (rnd.randrange(1, r) for _ in range(4))
    P, Q = G1.gen, G2.gen
    mul1 = lambda k: G1.amul(P, k % r)
    mul2 = lambda k: G2.amul(Q, k % r)
    neg = G1.aneg
    flip = lambda pt: (pt[0], (-pt[1]) % curve.q)
    admitted = [
        ("bilinear", [(mul1(a), mul2(b)), (neg(mul1(a * b)), Q)]),
        ("bilinear_a0", [(mul1(0), mul2(b)), (neg(mul1(0)), Q)]),
        ("bilinear_off_by_one", [(mul1(a), mul2(b)), (neg(mul1(a * b + 1)), Q)]),
        ("generators_alone", [(P, Q)]),
        ("three", [(mul1(a), Q), (mul1(b), Q), (neg(mul1(a + b)), Q)]),
        ("four", [(mul1(a), mul2(b)), (mul1(c), mul2(d)), (neg(mul1(a * b)), Q), (neg(mul1(c * d)), Q)]),
        ("four_wrong", [(mul1(a), mul2(b)), (mul1(c), mul2(d)), (neg(mul1(a * b)), Q), (neg(mul1(c * d + 1)), Q)]),
        ("inf_g1_first", [(None, mul2(b)), (mul1(a), Q)]),
        ("inf_g2_first", [(mul1(a), None), (mul1(a), Q)]),
        ("inf_g1_second", [(mul1(a), mul2(b)), (None, Q)]),
        ("inf_g2_second", [(mul1(a), mul2(b)), (neg(mul1(a * b)), None)]),
        ("inf_everywhere", [(None, None), (None, None)]),
        ("inf_then_one", [(None, mul2(c)), (mul1(a), mul2(b)), (neg(mul1(a * b)), Q)]),
        ("one_around_inf_g2", [(mul1(a), mul2(b)), (mul1(c), None), (neg(mul1(a * b)), Q)]),
        ("one_then_inf", [(mul1(a), mul2(b)), (neg(mul1(a * b)), Q), (None, None)]),
        ("other_torsion_point", [(flip(mul1(a)), mul2(b)), (neg(mul1(a * b)), Q)]),      # y -> p - y: on the curve, another point of order r
    ]
    cases = [(name, pairs, 1 if ctx.pairing_product_is_one(pairs) else 0) for name, pairs in admitted]
    assert [v for _, _, v in cases] == [1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0], [(n, v) for n, _, v in cases]
    good = [(mul1(a), mul2(b)), (neg(mul1(a * b)), Q)]
    refused = [("off_twist_subgroup", [(mul1(a), off_subgroup(curve, G2, 2)), good[1]]),
               ("off_curve_g1", [((mul1(a)[0], (mul1(a)[1] + 1) % curve.q), mul2(b)), good[1]]),
               ("off_curve_g2", [(mul1(a), (mul2(b)[0], (mul2(b)[1][0], (mul2(b)[1][1] + 1) % curve.q))), good[1]])]
    if curve is not BN254:
        refused.append(("off_curve_subgroup", [(off_subgroup(curve, G1, 1), mul2(b)), good[1]]))
    # a refused point next to a point at infinity: the pair is skipped by the product but the item is still refused
    refused.append(("refused_beside_infinity", [(None, off_subgroup(curve, G2, 2)), good[1]]))
    cases += [(name, pairs, 0) for name, pairs in refused]
    _primitive[ci] = cases
    return cases


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ci", range(3), ids=[c[0].name for c in CURVES])
def test_pairing_products_against_the_oracle(contexts, ci, backend):
    curve, cid = CURVES[ci][0], CURVES[ci][1]
    dev = contexts(backend)
    cases = primitive_cases(ci)
    for npairs in sorted({len(p) for _, p, _ in cases}):
        sel = [(n, p, v) for n, p, v in cases if len(p) == npairs]
        got = run_items(dev, curve, cid, [p for _, p, _ in sel])
        assert got == [v for _, _, v in sel], (curve.name, [n for n, _, _ in sel], got)


@pytest.mark.parametrize("backend", BACKENDS)
def test_item_counts_around_a_wavefront(contexts, backend):
    """0, 1, 2, G - 1, G, G + 1, 2 G + 1 items (G = 8: one wavefront, which is one workgroup), verdicts by construction: item i is
    e(a_i P, b_i Q) e(-(a_i b_i + [i % 3 == 1]) P, Q), and every position of every count is looked at."""
    curve, cid = BN254, 0
    G1, G2 = groups_of(curve)
    dev = contexts(backend)
    rnd = random.Random(77)
    items, want = [], []
    for i in range(2 * G + 1):
        a, b = rnd.randrange(1, curve.r), rnd.randrange(1, curve.r)
        bad = i % 3 == 1
        items.append([(G1.amul(G1.gen, a), G2.amul(G2.gen, b)), (G1.aneg(G1.amul(G1.gen, (a * b + bad) % curve.r)), G2.gen)])
        want.append(0 if bad else 1)
    for count in (1, 2, G - 1, G, G + 1, 2 * G + 1):
        assert run_items(dev, curve, cid, items[:count]) == want[:count], count
    assert dev.lib.L.zkhip_pairing_products(dev.h, cid, 0, 2, None, None, None) == 0          # count == 0: ZKHIP_OK, nothing is touched


@pytest.mark.parametrize("backend", BACKENDS)
def test_reference_mpc_fixture_points(contexts, backend, golden_dir):
    """The points of the reference's MPC fixture, with the verdicts tests/test_verify.py holds the host verifier to."""
    d = json.load(open(os.path.join(golden_dir, "phase1radix2m2_points.json")))
    G1, _ = groups(BN254)
    p1 = lambda v: (int(v[0]), int(v[1]))
    p2 = lambda v: ((int(v[0][0]), int(v[0][1])), (int(v[1][0]), int(v[1][1])))
    cg1, cg2 = [p1(v) for v in d["coeffs_g1"]], [p2(v) for v in d["coeffs_g2"]]
    ag1 = [p1(v) for v in d["alpha_coeffs_g1"]]
    two = [
        ([(cg1[1], BN254.g2), (G1.aneg(BN254.g1), cg2[1])], 1),
        ([(ag1[2], BN254.g2), (G1.aneg(p1(d["alpha_g1"])), cg2[2])], 1),
        ([(p1(d["beta_g1"]), BN254.g2), (G1.aneg(BN254.g1), p2(d["beta_g2"]))], 1),
        ([(cg1[1], BN254.g2), (G1.aneg(BN254.g1), cg2[2])], 0),
    ]
    dev = contexts(backend)
    assert run_items(dev, BN254, 0, [p for p, _ in two]) == [v for _, v in two]
    assert run_items(dev, BN254, 0, [two[0][0] + two[1][0] + two[2][0]]) == [1]              # six pairs in one item


def _gm17_items(curve, vk, proof, inputs):
    """the two products of ark-gm17's check (zokrates_proof_systems/src/scheme/gm17.rs:170-195) as items of the primitive; the
    sums A + g_alpha, B + h_beta and the input combination by the oracle's group law"""
    G1, G2 = groups_of(curve)
    psi = G1.to_jac(vk["query"][0])
    for x, base in zip(inputs, vk["query"][1:]):
        psi = G1.add(psi, G1.mul(G1.to_jac(base), x % curve.r))
    psi = G1.to_affine(psi)
    A, B, C = proof
    first = [(vk["g_alpha"], vk["h_beta"]), (psi, vk["h_gamma"]), (C, vk["h"]), (G1.aneg(G1.aadd(A, vk["g_alpha"])), G2.aadd(B, vk["h_beta"]))]
    second = [(A, vk["h_gamma"]), (G1.aneg(vk["g_gamma"]), B)]
    return first, second


@pytest.mark.parametrize("backend", BACKENDS)
def test_reference_gm17_proofs_over_bls12_377(contexts, backend, golden_dir):
    """Bytes the reference's ark backend produced (GM17, BLS12-377): both products of every triple are 1 on the device, and the
    first one is not once an input is incremented."""
    curve = bls377_ref.CURVE
    g1 = lambda a, i: (int(a[i], 0) if isinstance(a[i], str) else int(a[i]), int(a[i + 1], 0) if isinstance(a[i + 1], str) else int(a[i + 1]))
    g2 = lambda a, i: (g1(a, i), g1(a, i + 2))
    triples = []
    d = json.load(open(os.path.join(golden_dir, "gm17_bls12_377_triple.json")))
    h1 = lambda v: (int(v[0], 16), int(v[1], 16))
    h2 = lambda v: (h1(v[0]), h1(v[1]))
    v = d["vk"]
    triples.append(({"h": h2(v["h"]), "g_alpha": h1(v["g_alpha"]), "h_beta": h2(v["h_beta"]), "g_gamma": h1(v["g_gamma"]), "h_gamma": h2(v["h_gamma"]),
                     "query": [h1(q) for q in v["query"]]}, (h1(d["proof"]["a"]), h2(d["proof"]["b"]), h1(d["proof"]["c"])), [int(x, 16) for x in d["inputs"]]))
    e = json.load(open(os.path.join(golden_dir, "gm17_bls12_377_embed_triples.json")))
    for t in e["triples"]:
        pr, v, n_in = t["proof"], t["vk"], len(t["inputs"])
        triples.append(({"h": g2(v, 0), "g_alpha": g1(v, 4), "h_beta": g2(v, 6), "g_gamma": g1(v, 10), "h_gamma": g2(v, 12),
                         "query": [g1(v, 16 + 2 * i) for i in range(n_in + 1)]}, (g1(pr, 0), g2(pr, 2), g1(pr, 6)), [int(x) for x in t["inputs"]]))
    assert len(triples) == 4
    firsts, seconds, want = [], [], []
    for vk, proof, inputs in triples:
        f, s = _gm17_items(curve, vk, proof, inputs)
        firsts.append(f); seconds.append(s); want.append(1)
        changed = list(inputs)
        changed[-1] = (changed[-1] + 1) % curve.r
        firsts.append(_gm17_items(curve, vk, proof, changed)[0]); want.append(0)
    dev = contexts(backend)
    assert run_items(dev, curve, 2, firsts) == want
    assert run_items(dev, curve, 2, seconds) == [1] * len(seconds)


# ---------------------------------------------------------------- errors
@pytest.mark.parametrize("backend", BACKENDS)
def test_errors(contexts, backend):
    dev = contexts(backend)
    for curve, cid, _, _ in CURVES:
        G1, G2 = groups_of(curve)
        good = [(G1.gen, G2.gen), (G1.aneg(G1.gen), G2.gen)]
        items = [good, good, good]
        # a coordinate equal to p in item 1 (pair 1's G2 point), and a later one in item 2: the lowest is named, nothing is written
        bad_q = ((G2.gen[0][0], curve.q), G2.gen[1])
        items[1] = [good[0], (good[1][0], bad_q)]
        items[2] = [((curve.q, G1.gen[1]), G2.gen), good[1]]
        with pytest.raises(native.ZkhipError) as e:
            run_items(dev, curve, cid, items)
        assert e.value.code == -2 and "item 1, pair 1" in str(e.value) and "G2" in str(e.value), str(e.value)
        assert list(dev.last_ok) == [0xff] * 3
        items[1] = good
        with pytest.raises(native.ZkhipError) as e:
            run_items(dev, curve, cid, items)
        assert e.value.code == -2 and "item 2, pair 0" in str(e.value) and "G1" in str(e.value), str(e.value)
        assert list(dev.last_ok) == [0xff] * 3
        # (p - 1 is canonical: off the curve, verdict 0, no error)
        items[2] = [((curve.q - 1, G1.gen[1]), G2.gen), good[1]]
        assert run_items(dev, curve, cid, items) == [1, 1, 0]
    L = dev.lib.L
    one = np.zeros(4 * 48 + 1, dtype=np.uint8)
    p = lambda a: a.ctypes.data
    assert L.zkhip_pairing_products(dev.h, 0, 1, 1, None, p(one), p(one)) == -1              # null pointers
    assert L.zkhip_pairing_products(dev.h, 0, 1, 1, p(one), None, p(one)) == -1
    assert L.zkhip_pairing_products(dev.h, 0, 1, 1, p(one), p(one), None) == -1
    assert L.zkhip_pairing_products(None, 0, 1, 1, p(one), p(one), p(one)) == -1
    assert L.zkhip_pairing_products(dev.h, 0, 1, 0, p(one), p(one), p(one)) == -1            # pairs per item: 1 .. 8
    assert L.zkhip_pairing_products(dev.h, 0, 1, 9, p(one), p(one), p(one)) == -1
    assert L.zkhip_pairing_products(dev.h, 7, 1, 1, p(one), p(one), p(one)) == -1            # no such curve
    assert L.zkhip_pairing_products(dev.h, 7, 0, 1, None, None, None) == -1
    limbs = np.zeros((1, 6, 2, 9), dtype=np.uint32)
    assert L.zkhip_tower_op(dev.h, 0, 6, 1, p(limbs), p(limbs), p(limbs)) == -1              # no such op
    assert L.zkhip_tower_op(dev.h, 0, 0, 1, None, p(limbs), p(limbs)) == -1


# ---------------------------------------------------------------- the verifiers: the project's own proofs
INPUT_CHUNK = 64           # inputs one round of k_input_combination takes (csrc/pairing.cuh): l = 65 needs a second round
FR = {0: BN254.r, 1: BLS12_381.r, 2: bls377_ref.R}


def tiny_system(ctx, cid, n_pub):
    """z = (1, x_1 .. x_np | w1, w2, w3): x_i * 1 = x_i for every public input, w1 * w1 = w2, w2 * w1 = w3.  Domain 2^3 for np <= 5"""
    one = (1).to_bytes(32, "little")
    rows = [((i,), (0,), (i,)) for i in range(1, n_pub + 1)] + [((n_pub + 1,), (n_pub + 1,), (n_pub + 2,)), ((n_pub + 2,), (n_pub + 1,), (n_pub + 3,))]
    mats = []
    for k in range(3):
        cols = [r[k][0] for r in rows]
        mats.append((np.arange(len(rows) + 1, dtype=np.uint64), np.array(cols, dtype=np.uint32), np.frombuffer(one * len(cols), dtype=np.uint8)))
    return native.ConstraintSystem(ctx, cid, len(rows), n_pub + 1, 3, mats)


def tiny_assignment(cid, n_pub, seed):
    rnd = random.Random(seed)
    r = FR[cid]
    xs = [rnd.randrange(r) for _ in range(n_pub)]
    w1 = rnd.randrange(1, r)
    z = [1] + xs + [w1, w1 * w1 % r, w1 * w1 % r * w1 % r]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in z), dtype=np.uint8), xs


def flip_y(rec, nb, at, comps, q):
    """the record with the y of the point at byte `at` negated mod q (comps = 1: G1, 2: G2): another point of order r"""
    out = bytearray(rec)
    for c in range(comps):
        o = at + (comps + c) * nb
        y = int.from_bytes(out[o:o + nb], "little")
        out[o:o + nb] = ((q - y) % q).to_bytes(nb, "little")
    return bytes(out)


def inputs_bytes(xss):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for xs in xss for x in xs), dtype=np.uint8)


def make_proofs(dev, cid, scheme, n_pub, nproofs, tox_seed=0xC0FFEE):
    from zokrates_amd import synth
    cs = tiny_system(dev, cid, n_pub)
    tox = synth.toxic_waste(cid, seed=tox_seed)
    if scheme == "g16":
        raw = native.setup_g16(dev, cs, tox)
    else:
        raw = native.setup_gm17(dev, cs, (tox[0], tox[1], 1, tox[4]))
    pk = native.ProvingKey(dev, cid, raw, scheme=scheme)
    proofs, inputs = [], []
    for k in range(nproofs):
        z, xs = tiny_assignment(cid, n_pub, 1000 * n_pub + k)
        blind = (0, 0, 0) if k == 1 else (11 + k, 7 * k + 3, 5 * k + 2)          # proof 1: r = s = 0 (GM17: d1 = d2 = r = 0)
        if scheme == "g16":
            proofs.append(native.prove_g16(dev, pk, cs, z, blind[0], blind[1]))
        else:
            proofs.append(native.prove_gm17(dev, pk, cs, z, *blind))
        inputs.append(xs)
    pk.close()
    cs.close()
    return raw, proofs, inputs


# (the emulator half takes bn128 alone: a dozen batches of two workgroups are a minute per BLS curve there, seconds on the device;
# the emulator sees the BLS verifiers through the reference's triples and the BLS pairings through the primitive's cases)
@pytest.mark.parametrize("ci,backend", [(0, "emu")] + [pytest.param(ci, "gpu", marks=pytest.mark.gpu) for ci in range(3)],
                         ids=["bn128-emu"] + [c[0].name + "-gpu" for c in CURVES])
@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_own_proofs_and_their_mutations(contexts, ci, scheme, backend):
    """G + 1 proofs of the project's prover (three distinct ones, one of them with every blinding scalar 0, repeated) verify; then ONE
    item's A, B, C or input is altered — another point of order r, another input — and that item alone turns 0; two items swapped
    against their inputs turn 0, they alone; under the key of another setup all are 0."""
    curve, cid = CURVES[ci][0], CURVES[ci][1]
    nb = curve.fq_bytes
    dev = contexts(backend)
    verify = native.verify_g16_batch if scheme == "g16" else native.verify_gm17_batch
    raw, proofs, inputs = make_proofs(dev, cid, scheme, 5, 3)
    vk = native.VerificationKey(dev, cid, raw, scheme=scheme)
    assert vk.l == 5
    n = G + 1
    batch = [proofs[i % 3] for i in range(n)]
    ins = [inputs[i % 3] for i in range(n)]
    assert list(verify(dev, vk, batch, inputs_bytes(ins))) == [1] * n
    victim = 4
    for name, at, comps in (("A", 0, 1), ("B", 2 * nb, 2), ("C", 6 * nb, 1)):
        mutated = list(batch)
        mutated[victim] = flip_y(batch[victim], nb, at, comps, curve.q)
        assert list(verify(dev, vk, mutated, inputs_bytes(ins))) == [0 if i == victim else 1 for i in range(n)], name
    changed = [list(x) for x in ins]
    changed[victim][2] = (changed[victim][2] + 1) % curve.r
    assert list(verify(dev, vk, batch, inputs_bytes(changed))) == [0 if i == victim else 1 for i in range(n)]
    swapped = list(ins)
    swapped[3], swapped[4] = ins[4], ins[3]                    # items 3 and 4 hold different proofs (3 % 3 != 4 % 3)
    assert list(verify(dev, vk, batch, inputs_bytes(swapped))) == [0 if i in (3, 4) else 1 for i in range(n)]
    # an infinity flag on A, B or C: verdict 0 for that item, as the host verifier answers for the point it is handed then
    for flag in range(3):
        flagged = list(batch)
        rec = bytearray(batch[victim]); rec[8 * nb + flag] = 1
        flagged[victim] = bytes(rec)
        assert list(verify(dev, vk, flagged, inputs_bytes(ins))) == [0 if i == victim else 1 for i in range(n)], flag
    other_raw, _, _ = make_proofs(dev, cid, scheme, 5, 0, tox_seed=0xBEEF)
    other = native.VerificationKey(dev, cid, other_raw, scheme=scheme)
    assert list(verify(dev, other, batch, inputs_bytes(ins))) == [0] * n
    # errors: a coordinate equal to p, an input equal to r — ZKHIP_ERR_PARSE naming the item, no verdict written
    rec = bytearray(batch[2]); rec[6 * nb:7 * nb] = curve.q.to_bytes(nb, "little")
    with pytest.raises(native.ZkhipError) as e:
        verify(dev, vk, batch[:2] + [bytes(rec)] + batch[3:], inputs_bytes(ins))
    assert e.value.code == -2 and "item 2" in str(e.value) and " C " in str(e.value), str(e.value)
    assert list(dev.last_ok) == [0xff] * n
    big = [list(x) for x in ins]
    big[5][4] = curve.r
    big[7][0] = curve.r
    with pytest.raises(native.ZkhipError) as e:
        verify(dev, vk, batch, inputs_bytes(big))
    assert e.value.code == -2 and "item 5" in str(e.value) and "input 4" in str(e.value), str(e.value)
    assert list(dev.last_ok) == [0xff] * n
    # the wrong call for the key, a truncated key, null pointers, no proofs
    wrong = native.verify_gm17_batch if scheme == "g16" else native.verify_g16_batch
    with pytest.raises(native.ZkhipError) as e:
        wrong(dev, vk, batch, inputs_bytes(ins))
    assert e.value.code == -1 and "verifying key was handed" in str(e.value)
    fixed = (2 if scheme == "gm17" else 1) * 2 * nb + 3 * 4 * nb
    for cut in (fixed + 8 + 6 * 2 * nb - 1, fixed + 7, 10):
        with pytest.raises(native.ZkhipError) as e:
            native.VerificationKey(dev, cid, raw[:cut], scheme=scheme)
        assert e.value.code == -2, cut
    L = dev.lib.L
    fn = L.zkhip_verify_g16_batch if scheme == "g16" else L.zkhip_verify_gm17_batch
    ok = np.full(1, 0xff, dtype=np.uint8)
    one = np.frombuffer(batch[0], dtype=np.uint8)
    assert fn(dev.h, vk.h, 1, None, inputs_bytes(ins[:1]).ctypes.data, ok.ctypes.data) == -1
    assert fn(dev.h, vk.h, 1, one.ctypes.data, None, ok.ctypes.data) == -1
    assert fn(dev.h, vk.h, 1, one.ctypes.data, inputs_bytes(ins[:1]).ctypes.data, None) == -1
    assert fn(dev.h, None, 1, one.ctypes.data, inputs_bytes(ins[:1]).ctypes.data, ok.ctypes.data) == -1
    assert fn(dev.h, vk.h, 0, None, None, None) == 0 and ok[0] == 0xff
    vk.close(); other.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("scheme", ["g16", "gm17"])
@pytest.mark.parametrize("n_pub", [0, 1, INPUT_CHUNK + 1])
def test_input_counts(contexts, n_pub, scheme, backend):
    """l = 0, 1 and one more than a round of the input combination takes (5 is the other tests'), bn128, both schemes: two proofs
    verify, and with the LAST input of the second changed it does not."""
    dev = contexts(backend)
    verify = native.verify_g16_batch if scheme == "g16" else native.verify_gm17_batch
    raw, proofs, inputs = make_proofs(dev, 0, scheme, n_pub, 2)
    vk = native.VerificationKey(dev, 0, raw, scheme=scheme)
    assert vk.l == n_pub
    assert list(verify(dev, vk, proofs, inputs_bytes(inputs))) == [1, 1]
    if n_pub:
        changed = [list(x) for x in inputs]
        changed[1][-1] = (changed[1][-1] + 1) % BN254.r
        assert list(verify(dev, vk, proofs, inputs_bytes(changed))) == [1, 0]
    vk.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_reference_gm17_proofs_through_the_verifier(contexts, backend, golden_dir):
    """The reference's own GM17 / BLS12-377 triples through zkhip_verify_gm17_batch: its verifying key in ark's byte layout, its
    proof in the proof record; each verifies, and with one input incremented it does not."""
    curve, nb = bls377_ref.CURVE, 48
    le = lambda v: int(v).to_bytes(nb, "little")
    b1 = lambda P: le(P[0]) + le(P[1])
    b2 = lambda Q: le(Q[0][0]) + le(Q[0][1]) + le(Q[1][0]) + le(Q[1][1])
    num = lambda x: int(x, 0) if isinstance(x, str) and x.startswith("0x") else int(x, 16) if isinstance(x, str) and not x.isdigit() else int(x)
    g1 = lambda a, i: (num(a[i]), num(a[i + 1]))
    g2 = lambda a, i: (g1(a, i), g1(a, i + 2))
    h1 = lambda v: (int(v[0], 16), int(v[1], 16))
    h2 = lambda v: (h1(v[0]), h1(v[1]))
    triples = []
    d = json.load(open(os.path.join(golden_dir, "gm17_bls12_377_triple.json")))
    v = d["vk"]
    triples.append(((h2(v["h"]), h1(v["g_alpha"]), h2(v["h_beta"]), h1(v["g_gamma"]), h2(v["h_gamma"]), [h1(q) for q in v["query"]]),
                    (h1(d["proof"]["a"]), h2(d["proof"]["b"]), h1(d["proof"]["c"])), [int(x, 16) for x in d["inputs"]]))
    e = json.load(open(os.path.join(golden_dir, "gm17_bls12_377_embed_triples.json")))
    for t in e["triples"]:
        pr, v, n_in = t["proof"], t["vk"], len(t["inputs"])
        triples.append(((g2(v, 0), g1(v, 4), g2(v, 6), g1(v, 10), g2(v, 12), [g1(v, 16 + 2 * i) for i in range(n_in + 1)]),
                        (g1(pr, 0), g2(pr, 2), g1(pr, 6)), [int(x) for x in t["inputs"]]))
    dev = contexts(backend)
    for (h, g_alpha, h_beta, g_gamma, h_gamma, query), (A, B, C), inputs in triples:
        key = b2(h) + b1(g_alpha) + b2(h_beta) + b1(g_gamma) + b2(h_gamma) + len(query).to_bytes(8, "little") + b"".join(b1(q) for q in query)
        vk = native.VerificationKey(dev, 2, np.frombuffer(key, dtype=np.uint8), scheme="gm17")
        assert vk.l == len(inputs)
        rec = b1(A) + b2(B) + b1(C) + bytes(3)
        changed = list(inputs)
        changed[-1] = (changed[-1] + 1) % curve.r
        assert list(native.verify_gm17_batch(dev, vk, [rec, rec], inputs_bytes([inputs, changed]))) == [1, 0]
        vk.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_with_a_queue_open_and_a_split_proof_pending(contexts, backend):
    """Verify calls between the submits and collects of an open proof queue: the collected bytes are those of the same submits
    without the calls in between, and they verify.  With a split proof pending the calls are refused (ZKHIP_ERR_BAD_ARG) and the
    split proof then ends with its usual bytes."""
    from zokrates_amd import synth
    dev = contexts(backend)
    circ = synth.circuit(0, 4, seed=0xA11CE)
    cs = native.ConstraintSystem(dev, 0, circ.n, circ.l, circ.w, circ.mats())
    raw = native.setup_g16(dev, cs, synth.toxic_waste(0))
    pk = native.ProvingKey(dev, 0, raw)
    vk = native.VerificationKey(dev, 0, raw)
    zs = [circ.assignment(500 + i) for i in range(3)]
    rs = [(3 + i, 9 + 2 * i) for i in range(3)]
    pub = lambda z: np.frombuffer(z, dtype=np.uint8)[32:32 * circ.l]
    plain = [native.prove_g16(dev, pk, cs, z, r, s) for z, (r, s) in zip(zs, rs)]
    assert list(native.verify_g16_batch(dev, vk, plain, np.concatenate([pub(z) for z in zs]))) == [1, 1, 1]
    with native.ProofQueue(dev, pk, cs) as q:
        got = []
        for i, (z, (r, s)) in enumerate(zip(zs, rs)):
            q.submit(z, (r, s))
            assert list(native.verify_g16_batch(dev, vk, plain[:i + 1], np.concatenate([pub(x) for x in zs[:i + 1]]))) == [1] * (i + 1)
        for i in range(3):
            got.append(q.collect()[1])
            assert list(native.verify_g16_batch(dev, vk, got, np.concatenate([pub(x) for x in zs[:i + 1]]))) == [1] * (i + 1)
    assert got == plain
    # a split proof pending (two contexts, a shard of the key each): refused, and the split proof then ends with its usual bytes
    ctx2 = native.Context(0, emu_library()) if backend == "emu" else native.Context(0)
    cs2 = native.ConstraintSystem(ctx2, 0, circ.n, circ.l, circ.w, circ.mats())
    ranks = [(dev, native.ProvingKey(dev, 0, raw, rank=0, world=2), cs), (ctx2, native.ProvingKey(ctx2, 0, raw, rank=1, world=2), cs2)]
    for c, S, sys_ in ranks:
        S.bind_shard(sys_, raw)
    halves = [native.prove_g16_split_begin(c, S, sys_, zs[0], rs[0][0], rs[0][1], k) for k, (c, S, sys_) in enumerate(ranks)]
    with pytest.raises(native.ZkhipError) as e:
        native.verify_g16_batch(dev, vk, plain, np.concatenate([pub(z) for z in zs]))
    assert e.value.code == -1 and "split proof is pending" in str(e.value)
    assert list(dev.last_ok) == [0xff] * 3
    with pytest.raises(native.ZkhipError) as e:
        dev.pairing_products(0, 1, np.frombuffer(rec1(BN254.g1, 32), dtype=np.uint8), np.frombuffer(rec2(BN254.g2, 32), dtype=np.uint8))
    assert e.value.code == -1
    with pytest.raises(native.ZkhipError) as e:
        native.VerificationKey(dev, 0, raw)
    assert e.value.code == -1
    parts = [native.prove_g16_split_end(c, S, sys_, halves[1 - k]) for k, (c, S, sys_) in enumerate(ranks)]
    assert native.combine_g16(dev, ranks[0][1], parts, rs[0][0], rs[0][1]) == plain[0]
    assert list(native.verify_g16_batch(dev, vk, plain[:1], pub(zs[0]))) == [1]
    ranks[0][1].close(); ranks[1][1].close(); cs2.close(); ctx2.close()
    vk.close(); pk.close(); cs.close()


# ---------------------------------------------------------------- the host layer: zkhip-cli on the emulator
@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_cli_verify_on_the_device_says_what_the_host_verifier_says(tmp_path, scheme):
    """`zkhip-cli verify --device` (Hip::load_verification_key, Hip::verify_batch) against `zkhip-cli verify`: the same text and exit
    status for a proof that passes, for one whose input was changed (FAILED), for one whose coordinate is the field modulus and for
    one with an input too many (both: an error, status 1); `generate-proof --verify --device-verify` accepts the proof it writes."""
    import test_verify as tv
    env = tv._env()
    d = str(tmp_path)
    tv._program_files(d, BN254)
    p = lambda name: os.path.join(d, name)
    assert tv._run(["setup", "-i", p("out"), "-p", p("proving.key"), "-v", p("verification.key"), "-s", scheme, "--entropy", "dv"], env).returncode == 0
    r = tv._run(["generate-proof", "-i", p("out"), "-w", p("witness"), "-p", p("proving.key"), "-j", p("proof.json"), "-s", scheme, "--verify", "--device-verify"], env)
    assert r.returncode == 0 and "verified against the verification key" in r.stdout, (r.stdout, r.stderr)
    good = json.load(open(p("proof.json")))
    changed = dict(good, inputs=[good["inputs"][0]] + [tv._hex(int(x, 16) + 1, 32) for x in good["inputs"][1:]])
    noncanon = json.loads(json.dumps(good))
    noncanon["proof"]["c"][0] = tv._hex(BN254.q, 32)
    extra = dict(good, inputs=good["inputs"] + [tv._hex(1, 32)])
    big = dict(good, inputs=good["inputs"][:-1] + [tv._hex(BN254.r, 32)])
    for name, doc, want in (("good", good, "PASSED"), ("changed", changed, "FAILED"), ("noncanon", noncanon, None), ("extra", extra, None), ("big", big, None)):
        json.dump(doc, open(p(name + ".json"), "w"))
        host = tv._run(["verify", "-v", p("verification.key"), "-j", p(name + ".json")], env)
        dev = tv._run(["verify", "-v", p("verification.key"), "-j", p(name + ".json"), "--device"], env)
        assert host.returncode == dev.returncode and host.stdout == dev.stdout, (name, host.stdout, host.stderr, dev.stdout, dev.stderr)
        if want:
            assert dev.returncode == 0 and dev.stdout.split()[-1] == want, (name, dev.stdout, dev.stderr)
        else:
            assert dev.returncode == 1 and dev.stderr.strip(), name


# ---------------------------------------------------------------- the host verifier as the truth: tests/host/device_verify.cpp
_program = {}


def host_program():
    """tests/host/device_verify.cpp against the emulator library and the compiled host layer"""
    if "exe" not in _program:
        import subprocess
        import tempfile
        from emu_util import EMU_DIR
        emu_library()
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        host = os.path.join(root, "zokrates_amd", "csrc", "host")
        exe = os.path.join(tempfile.mkdtemp(prefix="device_verify_"), "device_verify")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", os.path.join(root, "tests", "host", "device_verify.cpp"),
                               os.path.join(host, "backend.cpp"), os.path.join(host, "verify.cpp"), "-L" + EMU_DIR, "-lzkhip_emu", "-Wl,-rpath," + EMU_DIR, "-o", exe])
        _program["exe"] = exe
    return _program["exe"]


def run_program(args):
    import subprocess
    r = subprocess.run([host_program()] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("verdicts "), (r.stdout, r.stderr)
    return [int(c) for c in r.stdout.split()[1]]


def infinite_a_proof(dev, cid, n_pub, raw, z):
    """A proof whose A the PROVER leaves at infinity (its flag byte set by the device): the honest key with alpha_g1 and every
    a_query entry at infinity, as tests/test_degenerate_bases.py rewrites keys, and r = 0 — A = alpha + sum z_i a_i + r delta = O."""
    from oracle import formats
    curve = CURVES[cid][0]
    pk = formats.ark_pk_deserialize(curve, bytes(raw))
    pk["vk"]["alpha_g1"] = None
    pk["a_query"] = [None] * len(pk["a_query"])
    raw2 = np.frombuffer(formats.ark_pk_serialize(curve, pk), dtype=np.uint8)
    cs = tiny_system(dev, cid, n_pub)
    key = native.ProvingKey(dev, cid, raw2)
    rec = native.prove_g16(dev, key, cs, z, 0, 5)
    key.close(); cs.close()
    assert rec[8 * curve.fq_bytes] == 1 and rec[8 * curve.fq_bytes + 1] == 0, "the prover flags A, and A alone, as the point at infinity"
    return rec


@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_hip_verify_batch_against_the_host_verifier(contexts, tmp_path, scheme):
    """Case 4's whole mutation set as ONE batch through Hip::verify_batch and through zkhip_verify_*_batch, every verdict compared
    with the host `verify` inside tests/host/device_verify.cpp (which also gives a proof the tag of another curve and loads the key
    under another curve id), and the host's verdicts compared with what the construction says: four proofs (one with all blinding
    scalars 0), then A, B, C negated, an input changed, two items' inputs swapped and — Groth16 — a proof whose A the prover itself
    left at infinity; then all of them under the key of another setup."""
    curve, cid = BN254, 0
    nb = curve.fq_bytes
    dev = contexts("emu")
    raw, proofs, inputs = make_proofs(dev, cid, scheme, 5, 3)
    recs = [proofs[0], proofs[1], proofs[2], proofs[0]]
    ins = [inputs[0], inputs[1], inputs[2], inputs[0]]
    want = [1, 1, 1, 1]
    for at, comps in ((0, 1), (2 * nb, 2), (6 * nb, 1)):
        recs.append(flip_y(proofs[2], nb, at, comps, curve.q)); ins.append(inputs[2]); want.append(0)
    changed = list(inputs[1]); changed[3] = (changed[3] + 1) % curve.r
    recs.append(proofs[1]); ins.append(changed); want.append(0)
    recs += [proofs[0], proofs[1]]; ins += [inputs[1], inputs[0]]; want += [0, 0]
    if scheme == "g16":
        z, xs = tiny_assignment(cid, 5, 77)
        recs.append(infinite_a_proof(dev, cid, 5, raw, z)); ins.append(xs); want.append(0)
    files = {"key": bytes(raw), "records": b"".join(recs), "inputs": inputs_bytes(ins).tobytes()}
    other_raw, _, _ = make_proofs(dev, cid, scheme, 5, 0, tox_seed=0xBEEF)
    files["other"] = bytes(other_raw)
    for name, data in files.items():
        open(str(tmp_path / name), "wb").write(data)
    p = lambda name: str(tmp_path / name)
    assert run_program(["verify", cid, scheme, p("key"), p("records"), p("inputs"), 5]) == want
    assert run_program(["verify", cid, scheme, p("other"), p("records"), p("inputs"), 5]) == [0] * len(want)
    # the same batch through the binding: the device's verdicts are the host's
    vk = native.VerificationKey(dev, cid, raw, scheme=scheme)
    verify = native.verify_g16_batch if scheme == "g16" else native.verify_gm17_batch
    assert list(verify(dev, vk, recs, inputs_bytes(ins))) == want
    vk.close()


@pytest.mark.parametrize("ci", range(3), ids=[c[0].name for c in CURVES])
def test_pairing_products_against_the_host_verifier(ci, tmp_path):
    """The primitive's cases without a point at infinity (a hex coordinate cannot spell one) through tests/host/device_verify.cpp:
    zkhip_pairing_products against the host's pairing_product_is_one, item by item; where the host throws (a point outside its
    group) the device's verdict is 0.  The host's verdicts are the oracle's."""
    import test_verify as tv
    curve, cid = CURVES[ci][0], CURVES[ci][1]
    cases = [(n, pr, v) for n, pr, v in primitive_cases(ci) if all(P is not None and Q is not None for P, Q in pr)]
    assert len(cases) >= 9
    for npairs in sorted({len(pr) for _, pr, _ in cases}):
        sel = [(n, pr, v) for n, pr, v in cases if len(pr) == npairs]
        f = str(tmp_path / ("pairs%d.txt" % npairs))
        tv._pairs_file(f, [pq for _, pr, _ in sel for pq in pr], curve.fq_bytes)
        assert run_program(["pairs", cid, npairs, f]) == [v for _, _, v in sel], [n for n, _, _ in sel]


@pytest.mark.parametrize("backend", BACKENDS)
def test_curve_mismatch(contexts, backend):
    """A bn128 key under a BLS curve id and a BLS key under bn128's: refused at load (ZKHIP_ERR_PARSE), both schemes.  (A proof of
    another curve handed to Hip::verify_batch: tests/host/device_verify.cpp.)"""
    dev = contexts(backend)
    for scheme in ("g16", "gm17"):
        keys = {cid: make_proofs(dev, cid, scheme, 1, 0)[0] for cid in (0, 1)}
        for cid, other in ((0, 1), (0, 2), (1, 0)):
            with pytest.raises(native.ZkhipError) as e:
                native.VerificationKey(dev, other, keys[cid], scheme=scheme)
            assert e.value.code == -2, (scheme, cid, other, str(e.value))
        assert native.VerificationKey(dev, 0, keys[0], scheme=scheme).l == 1
