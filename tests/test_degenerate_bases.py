"""Repeated, opposite and infinite bases, where the branch-free mixed addition of the bucket accumulation cannot go.

k_msm_accum decides its one rare path — the running sum meets the same point again (a doubling), its opposite (a cancellation) or,
in the SKIP_INF = false kernel, a base at infinity — by a wavefront vote: if ANY lane has the case, all 64 run the general code for
that step, with their own ordinary operands.  The inputs here put such lanes and lanes in the other three states (starting a sum,
sitting out an infinite base, adding) into one wavefront on purpose, on every curve and in both groups, and place the boundaries
of the signed-digit recoding (raw == K, raw == K + 1, an all-ones window plus carry) in every window width used.

Every comparison is byte-exact against a reference: oracle.cpu (C++) for BN254 and BLS12-381, tests/bls377_ref.py (Python big
ints) for BLS12-377.  Nothing compares the device with itself or with the emulator.  Whether a path is reached is not assumed: a
Python restatement of the recoding (`recode`, written from the comment above k_msm_digits) counts, before each call, the buckets
that hold exactly one (P, P) or one (P, -P) group and the digit boundaries met, and the test asserts those counts.

CPU tests run on the emulator build (whose ZK_WAVE_ANY is a vote of the wave's 64 fibres); the `gpu` ones repeat them on the device
at sizes that fill several wavefronts."""
import collections
import functools
import random

import numpy as np
import pytest

import bls377_ref as ref
from oracle import cpu, formats
from oracle import curves as ocurves
from oracle import gm17 as ogm17
from oracle import groth16 as g16
from oracle.fields import BN254, BLS12_381
from zokrates_amd import native

from emu_util import emu_library
from size_ladder import adhoc_window, table_window      # the shape model: the widths msm_shape picks, without and with tables

CURVES = {0: BN254, 1: BLS12_381, 2: ref.CURVE}
RUN = 40                                   # length of the runs of equal and of alternating bases


def le(vals, nb=32):
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "little") for v in vals), dtype=np.uint8)


def group_of(curve_id, group):
    return (ocurves.groups(CURVES[curve_id]) if curve_id < 2 else ref.groups377())[group - 1]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0, emu_library())
    assert "EMULATOR" in c.describe()
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu_ctx():
    c = native.Context(0)
    assert "gfx950" in c.describe() and "EMULATOR" not in c.describe()
    yield c
    c.close()


# ------------------------------------------------------------------ the model: window width, recoding, edge scalars
def scalar_bits(curve):
    return curve.r.bit_length()            # Fr::Params::BITS (254, 255, 253)


def windows(curve, c):
    return (scalar_bits(curve) + 1 + c - 1) // c


def recode(k, c, W):
    """Signed digits of k, window by window: digit = raw + carry in, minus 2^c (and a carry out) when that exceeds K = 2^(c-1).
    -> [(digit, raw + carry in)]; digit 0 is dropped by the sort, digit d goes to bucket |d| - 1 with its sign."""
    K, full = 1 << (c - 1), 1 << c
    out, carry = [], 0
    for j in range(W):
        raw = ((k >> (j * c)) & (full - 1)) + carry
        if raw > K:
            out.append((raw - full, raw))
            carry = 1
        else:
            out.append((raw, raw))
            carry = 0
    assert carry == 0 and sum(d << (j * c) for j, (d, _) in enumerate(out)) == k
    return out


def edge_scalars(curve, c):
    """The scalars that put the recoding's boundaries into the windows of width c (values truncated below r)."""
    r = curve.r
    W = windows(curve, c)
    K, ones = 1 << (c - 1), (1 << c) - 1
    below_r = (1 << (r.bit_length() - 1)) - 1
    every = lambda w, sel=lambda j: True: sum(w << (j * c) for j in range(W) if sel(j)) & below_r
    straddling = [j for j in range(1, W - 1) if (j * c) // 32 != (j * c + c - 1) // 32]       # windows across a limb boundary
    aligned = [j for j in range(1, W - 1) if (j * c) % 32 == 0]                                # ... or starting at one (c = 8, 16)
    limb = (straddling or aligned)[0]
    return [0, 1, r - 1, every(K), every(K + 1), every(ones), every(ones, lambda j: j % 2 == 0), every(ones, lambda j: j % 2 == 1),
            ones, ones << (limb * c), (ones << ((W - 1) * c)) & below_r]


# ------------------------------------------------------------------ the generator
KINDS = ("PP", "PN", "PPN", "PQR", "PI", "II")


class Case:
    """n bases and scalars built of groups that share one scalar, and filler, for the window widths `widths`.

    One group per edge scalar of every width (the kinds in turn), `nrandom` groups (P, P) and as many (P, -P) with full-width random
    scalars, one group of every other kind and the two runs.  The layout (scalars and who sits where) is made first and tested on the
    model; the seed is the first for which the model's conditions hold, so that they hold by construction and not by luck."""

    def __init__(self, curve_id, group, n, widths, nrandom, seed):
        curve, G = CURVES[curve_id], group_of(curve_id, group)
        self.curve_id, self.group, self.n, self.curve, self.G, self.widths = curve_id, group, n, curve, G, tuple(widths)
        for attempt in range(16):
            self.seed = seed + 0x100 * attempt
            self._layout(random.Random(self.seed), nrandom)
            if all(self.covered(c) for c in self.widths):
                break
        else:
            raise AssertionError("no layout of %d points meets the model's conditions at the widths %s" % (n, self.widths))
        ser = formats.ser_g1 if group == 1 else formats.ser_g2
        self.point_bytes = len(ser(curve, None))
        self.scalar_bytes = le(self.ks)

    def _layout(self, rnd, nrandom):
        r, bits, n = self.curve.r, scalar_bits(self.curve), self.n
        edges = []
        for c in self.widths:
            edges += [k for k in edge_scalars(self.curve, c) if k not in edges]
        narrow = max(self.widths) < 8
        groups = [(KINDS[i % len(KINDS)], k) for i, k in enumerate(edges)]
        for kind in KINDS:                                  # full-width random scalars
            groups += [(kind, rnd.randrange(r)) for _ in range(nrandom if kind in ("PP", "PN") else 1)]
        # (under a narrow width every full-width scalar sits in every window's few buckets: there the runs take edge scalars)
        groups += [("RUN_EQ", edges[-3] if narrow else rnd.randrange(r)), ("RUN_ALT", edges[-2] if narrow else rnd.randrange(r))]
        sizes = {"PP": 2, "PN": 2, "PPN": 3, "PQR": 3, "PI": 2, "II": 2, "RUN_EQ": RUN, "RUN_ALT": RUN, "F": 1}
        used = sum(sizes[kind] for kind, _ in groups)
        assert 2 * used <= n, "the filler is at least half of all entries: %d of %d are groups" % (used, n)
        # filler: distinct bases, random scalars of random widths (the high windows of a narrow width stay thinly populated)
        groups += [("F", rnd.randrange(1 << rnd.randrange(1, bits)) % r) for _ in range(n - used)]
        rnd.shuffle(groups)
        self.ks, self.kinds, self.members = [], [], {kind: [] for kind in sizes}
        for kind, k in groups:
            self.members[kind].append(tuple(range(len(self.ks), len(self.ks) + sizes[kind])))
            self.kinds.append(kind)
            self.ks += [k] * sizes[kind]
        assert len(self.ks) == n
        self._walk_seed = rnd.randrange(1, r), rnd.randrange(1, r)
        if narrow:
            self._give_pairs_a_bucket(rnd, edges)

    def _give_pairs_a_bucket(self, rnd, edges):
        """The last step of a narrow-width layout.  With 2 to 16 buckets per window a pair has one to itself only in the thinly
        populated high windows, and a random scalar seldom has a digit there that nobody shares.  Pair by pair, the full-width
        random scalar (never an edge scalar) is replaced by the first of up to 256 fresh full-width draws some digit of which
        falls into a bucket no other entry uses; `held` counts the entries per bucket key with the pair itself taken out."""
        c, r = self.widths[0], self.curve.r
        W = windows(self.curve, c)
        keys_of = lambda k: [(j, abs(d) - 1) for j, (d, _) in enumerate(recode(k, c, W)) if d]
        held = collections.Counter(key for k in self.ks for key in keys_of(k))
        for kind in ("PP", "PN"):
            for i, j in self.members[kind]:
                if self.ks[i] in edges:
                    continue
                held.subtract(keys_of(self.ks[i]) * 2)
                for _ in range(256):
                    k = rnd.randrange(r)
                    if any(held[key] == 0 for key in keys_of(k)):
                        break
                held.update(keys_of(k) * 2)
                self.ks[i] = self.ks[j] = k

    @functools.cached_property
    def bases(self):
        """Distinct points from a walk of affine additions off two random multiples of the generator (n scalar multiplications
        would cost the Python side of a G2 case many seconds), laid out group by group."""
        G = self.G
        at, step = G.amul(G.gen, self._walk_seed[0]), G.amul(G.gen, self._walk_seed[1])
        out = []
        def fresh():
            nonlocal at
            at = G.aadd(at, step)
            assert at is not None
            return at
        for kind in self.kinds:
            P = fresh()
            out += {"PP": lambda: [P, P], "PN": lambda: [P, G.aneg(P)], "PPN": lambda: [P, P, G.aneg(P)], "PQR": lambda: [P, fresh(), fresh()],
                    "PI": lambda: [P, None], "II": lambda: [None, None], "RUN_EQ": lambda: [P] * RUN,
                    "RUN_ALT": lambda: [P if i % 2 == 0 else G.aneg(P) for i in range(RUN)], "F": lambda: [P]}[kind]()
        assert len(out) == self.n
        return out

    @functools.cached_property
    def base_bytes(self):
        ser = formats.ser_g1 if self.group == 1 else formats.ser_g2
        return np.frombuffer(b"".join(ser(self.curve, P) for P in self.bases), dtype=np.uint8)

    def coverage(self, c):
        """From the model alone: the bucket keys (window, bucket) whose entries are exactly one (P, P) group, the same for (P, -P),
        and which of the recoding's boundaries some window meets."""
        W = windows(self.curve, c)
        K, full = 1 << (c - 1), 1 << c
        keys, met = {}, set()
        for i, k in enumerate(self.ks):
            for j, (d, raw) in enumerate(recode(k, c, W)):
                if raw in (K, K + 1, full):
                    met.add({K: "raw == K", K + 1: "raw == K + 1", full: "raw == 2^c"}[raw])
                if d:
                    keys.setdefault((j, abs(d) - 1), []).append(i)
        held = [tuple(v) for v in keys.values()]
        pp, pn = set(self.members["PP"]), set(self.members["PN"])
        return sum(v in pp for v in held), sum(v in pn for v in held), met

    def covered(self, c):
        pp, pn, met = self.coverage(c)
        return min(pp, pn) >= (64 if c == 16 else 1) and len(met) == 3

    def check_coverage(self, c):
        assert c in self.widths
        pp, pn, met = self.coverage(c)
        need = 64 if c == 16 else 1
        assert pp >= need and pn >= need, "buckets holding exactly one (P, P) / (P, -P) group at c = %d: %d / %d" % (c, pp, pn)
        assert met == {"raw == K", "raw == K + 1", "raw == 2^c"}, (c, met)

    @functools.cached_property
    def want(self):
        """The reference's sum, in the bytes the library returns: the affine point, then a flag byte for the point at infinity."""
        if self.curve_id < 2:
            return bytes(cpu.msm(self.curve_id, self.group, self.base_bytes, self.scalar_bytes))
        S = self.G.to_affine(self.G.msm(self.bases, self.ks))
        ser = formats.ser_g1 if self.group == 1 else formats.ser_g2
        return bytes(self.point_bytes) + b"\x01" if S is None else ser(self.curve, S) + b"\x00"


@functools.lru_cache(maxsize=None)
def case(curve_id, group, n, wide):
    """Two cases per curve, group and size: one for the widths 8 and 16, with enough full-width groups for 64 buckets of each kind at
    16, and one for the narrow width an MSM of this size picks by itself (msm_c = 0), where 2 to 16 buckets per window leave a pair to
    itself only while few full-width scalars are about."""
    auto = adhoc_window(n, scalar_bits(CURVES[curve_id]))
    assert auto < 8
    return Case(curve_id, group, n, (8, 16) if wide else (auto,), 7 if wide else 3, 0xDE6E0000 + 32 * curve_id + 2 * group + wide)


def msm_everywhere(c, curve_id, group, n, n_own, slices=(1, 2, 8), modes=(1, 2)):
    """The ad-hoc MSM under every window width, slice length and way of meeting infinite bases, each case against ONE reference sum.
    Slices of one entry: every lane only starts a sum and the fold meets the equal and opposite partial sums (xyzz_add_from,
    msm_bucket_sum); of 2 and 8: the accumulation meets them."""
    try:
        for width in (0, 8, 16):
            cs = case(curve_id, group, n if width else n_own, width != 0)
            cs.check_coverage(width or cs.widths[0])            # a condition: the paths are reached, by the model
            c.tune("msm_c", width)
            for min_slice in slices:
                c.tune("msm_min_slice", min_slice)
                for mode in modes:
                    c.tune("skip_inf", mode)
                    got = c.msm(curve_id, group, cs.base_bytes, cs.scalar_bytes)
                    assert got == cs.want, (width, min_slice, mode)
    finally:
        c.tune("msm_c", 0)
        c.tune("msm_min_slice", 8)
        c.tune("skip_inf", 0)


def test_recoding_model():
    """The restatement itself: digits in [-K + 1, K], the boundaries where the comment above k_msm_digits puts them."""
    for c in (2, 5, 8, 16, 17):
        K, full = 1 << (c - 1), 1 << c
        W = windows(BN254, c)
        for k in edge_scalars(BN254, c) + [random.Random(c).randrange(BN254.r) for _ in range(20)]:
            assert all(-K < d <= K for d, _ in recode(k, c, W))
        assert recode(K, c, W)[0] == (K, K) and recode(K + 1, c, W)[:2] == [(K + 1 - full, K + 1), (1, 1)]
        assert recode(full * full - 1, c, W)[:3] == [(-1, full - 1), (0, full), (1, 1)]


# The sizes: (curve, group, n for the widths 8 and 16, n for the MSM's own width).  One group per edge scalar of two widths (about 20)
# and 18 of random scalars are some 90 entries, the two runs 80 more, and the filler doubles that: 360 is the smallest size at which
# the filler is half of all entries.  Under its own width an MSM of fewer than 512 points has windows of 2 or 3 bits, whose 2 or 4
# buckets the dozen full-width scalars of the edge list fill in every window: no pair has a bucket to itself below 512 points.
SIZES_EMU = [(cid, grp, 360, 512) for cid in (0, 1, 2) for grp in (1, 2)]
SIZES_GPU = [(cid, grp, n, n) for cid in (0, 1, 2) for grp, n in ((1, 2000), (2, 600))]
_ids = lambda v: "%s-G%d-%d" % (CURVES[v[0]].name, v[1], v[2])


@pytest.mark.parametrize("wide", [False, True], ids=["own-width", "8-and-16"])
@pytest.mark.parametrize("shape", SIZES_EMU + SIZES_GPU, ids=_ids)
def test_coverage_of_the_generated_cases(shape, wide):
    """The conditions the device tests rest on, from the model alone and without any library."""
    cs = case(shape[0], shape[1], shape[2] if wide else shape[3], wide)
    for c in cs.widths:
        cs.check_coverage(c)
    assert len(cs.members["F"]) * 2 >= cs.n
    assert len(cs.members["RUN_EQ"][0]) == len(cs.members["RUN_ALT"][0]) == RUN
    if shape in SIZES_EMU:
        assert all(cs.G.on_curve(P) for P in cs.bases)
        real = [P for P in cs.bases if P is not None]
        repeats = len(cs.members["PP"]) + len(cs.members["PPN"]) + (RUN - 1) + (RUN - 2)      # one per pair, and the two runs'
        assert len(set(real)) == len(real) - repeats, "everything else is distinct"


@pytest.mark.parametrize("shape", SIZES_EMU, ids=_ids)
def test_msm_structured_groups(ctx, shape):
    msm_everywhere(ctx, *shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SIZES_GPU, ids=_ids)
def test_gpu_msm_structured_groups(gpu_ctx, shape):
    msm_everywhere(gpu_ctx, *shape)


# ------------------------------------------------------------------ proofs over circuits with twin variables (honest keys)
def witness_values(curve, rnd, m_about, extra=6):
    """The common witness values of the groups, drawn like the scalars of the MSM cases: the edge lists of the key's own window
    width and of the widest one, and full-width random values."""
    vals = []
    for c in (table_window(m_about, scalar_bits(curve)), 17):
        vals += [k for k in edge_scalars(curve, c) if k not in vals]
    return vals + [rnd.randrange(curve.r) for _ in range(extra)]


SIGNS = {"twins": (1, 1), "opposite": (1, -1), "triple": (1, 1, -1), "no_b": (1, 1), "run": (1,) * RUN, "c_side": (1, 1, -1)}


def twin_system(curve, rnd, nfill, l=4):
    """A satisfied system in the style of test_random_circuits.random_system whose rows introduce groups of free variables with the
    same witness value and identical (`twins`, `run`), opposite (`opposite`: coefficients c and r - c) or mixed (`triple`: +, +, -)
    columns in A, B and C; twins that B never mentions (`no_b`: both b queries hold the point at infinity for them); and twins on the
    C side (`c_side`: C_k = y1 + y2 - y3 with y1 = y2 = y3).  The variables of a group occur in that one row only, and the row's
    fresh C variable takes the product, so the system stays satisfied.  -> (R1CS, z, [(kind, variables, signs)])."""
    r = curve.r
    z = [1] + [rnd.choice([0, 1, 2, rnd.randrange(r)]) for _ in range(l - 1)]
    pool = list(range(l))                       # the variables ordinary rows may mention: never a member of a group
    A, B, C, groups = [], [], [], []
    small = lambda: rnd.choice([1, r - 1, 2, rnd.randrange(1 << 64), rnd.randrange(r)])
    ev = lambda row: sum(c * z[j] for j, c in row) % r

    def lc(maxlen):
        cols = rnd.sample(pool, min(rnd.randrange(0, maxlen + 1), len(pool)))
        return [(c, small()) for c in cols]

    def fresh(v):
        z.append(v % r)
        return len(z) - 1

    def close_row(a, b):
        y = fresh(ev(a) * ev(b))
        pool.append(y)
        A.append(a); B.append(b); C.append([(y, 1)])

    def filler_row():
        a, b = lc(4), lc(3)
        if rnd.random() < 0.15:                 # 0 * b = 0 with an empty C row
            A.append([]); B.append(b); C.append([])
        else:
            close_row(a, b)

    def group_row(kind, v):
        sg = SIGNS[kind]
        if kind == "c_side":
            x, ys = fresh(v), [fresh(v) for _ in sg]
            A.append([(x, 1)]); B.append([(0, 1)]); C.append([(y, s % r) for y, s in zip(ys, sg)])
            groups.append((kind, ys, sg))
            return
        ca, cb = rnd.randrange(1, r), rnd.choice([1, 2, rnd.randrange(1, r)])
        xs = [fresh(v) for _ in sg]
        a = [(x, ca * s % r) for x, s in zip(xs, sg)] + lc(2)
        b = lc(3) if kind == "no_b" else [(x, cb * s % r) for x, s in zip(xs, sg)] + lc(2)
        close_row(a, b)
        groups.append((kind, xs, sg))

    kinds = ("twins", "opposite", "triple", "no_b", "c_side")
    values = witness_values(curve, rnd, 6 * nfill)
    rows = [("run", rnd.randrange(r))] + [(kinds[i % len(kinds)], v) for i, v in enumerate(values)] + [None] * nfill
    rnd.shuffle(rows)
    for row in [None, None] + rows:             # (two ordinary rows first: the pool has more than the public inputs)
        if row is None:
            filler_row()
        else:
            group_row(*row)
    cs = g16.R1CS(l=l, w=len(z) - l)
    cs.A, cs.B, cs.C = A, B, C
    assert cs.is_satisfied(z, r)
    return cs, z, groups


def csr(rows, nb=32):
    rp, col, val = [0], [], []
    for row in rows:
        for j, v in sorted(row):
            col.append(j); val.append(v)
        rp.append(len(col))
    return np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), le(val) if val else np.zeros(0, dtype=np.uint8)


def check_key_entries(curve_id, scheme, raw, cs, groups):
    """The builder did what it says: on the serialized key the entries of a group are equal, opposite or the point at infinity.
    Groth16: a_query, both b queries, l_query.  GM17 (SAP columns: A + B and A - B of the variable's rows): a_query, b_query and
    c_query_2 are infinite for the C-side twins only, c_query_1 (the witness variables') is finite everywhere."""
    curve = CURVES[curve_id]
    G1, G2 = group_of(curve_id, 1), group_of(curve_id, 2)
    if scheme == "g16":
        pk = formats.ark_pk_deserialize(curve, bytes(raw))
        queries = (("a_query", G1), ("b_g1_query", G1), ("b_g2_query", G2), ("l_query", G1))
    else:
        pk = gm17_pk_deserialize(curve, bytes(raw))
        queries = (("a_query", G1), ("b_query", G2), ("c_query_2", G1), ("c_query_1", G1))
    seen = collections.Counter()
    for kind, xs, sg in groups:
        seen[kind] += 1
        for name, G in queries:
            witness_only = name in ("l_query", "c_query_1")
            pts = [pk[name][x - (cs.l if witness_only else 0)] for x in xs]
            if scheme == "g16":
                infinite = kind == "c_side" and name != "l_query" or kind == "no_b" and name.startswith("b_")
            else:
                infinite = kind == "c_side" and not witness_only
            if infinite:
                assert all(P is None for P in pts), (kind, name)
            else:
                assert pts[0] is not None, (kind, name)
                assert all(P == (pts[0] if s == sg[0] else G.aneg(pts[0])) for P, s in zip(pts, sg)), (kind, name)
    assert seen["run"] == 1 and all(seen[k] >= 3 for k in ("twins", "opposite", "triple", "no_b", "c_side")), seen


class Refs:
    """The two references of a scheme over one system, as bytes: the C++ oracle for BN254 and BLS12-381, the Python one for BLS12-377."""

    def __init__(self, curve_id, cs, z, mats, scheme, seed):
        self.curve_id, self.cs, self.z, self.scheme, self.curve = curve_id, cs, z, scheme, CURVES[curve_id]
        self.zb = le(z)
        self.tox = (g16.Toxic if scheme == "g16" else ogm17.Toxic).from_seed(self.curve, seed)
        if curve_id < 2:
            self.oc = cpu.Circuit.from_csr(curve_id, cs.n, cs.l, cs.w, mats)
            self.tb = cpu.toxic_bytes(self.tox) if scheme == "g16" else cpu.gm17_toxic_bytes(self.tox)

    def toxic(self):
        t = self.tox
        return (t.alpha, t.beta, t.gamma, t.delta, t.tau) if self.scheme == "g16" else (t.alpha, t.beta, t.gamma, t.t)

    def key(self):
        if self.curve_id < 2:
            return (cpu.ProvingKey if self.scheme == "g16" else cpu.Gm17ProvingKey).setup(self.oc, self.tb).serialize().tobytes()
        if self.scheme == "g16":
            return formats.ark_pk_serialize(self.curve, ref.g16_setup(self.cs, self.tox)[0])
        return ogm17.pk_serialize(self.curve, ref.gm17_setup(self.cs, self.tox)[0])

    def closed_form(self, rnd3):
        if self.scheme == "g16":
            a, b = rnd3
            if self.curve_id < 2:
                return cpu.trapdoor(self.oc, self.tb, self.zb, a, b)
            return formats.proof_raw(self.curve, ref.g16_trapdoor(self.cs, self.tox, self.z, a, b))
        d1, _, r_ = rnd3
        if self.curve_id < 2:
            return cpu.gm17_trapdoor(self.oc, self.tb, self.zb, d1, r_)
        return formats.proof_raw(self.curve, ref.gm17_trapdoor(self.cs, self.tox, self.z, d1, r_))

    def algorithmic(self, raw, rnd3):
        """The algorithmic prover over the key BYTES `raw` (whatever made them)."""
        if self.scheme == "g16":
            if self.curve_id < 2:
                return cpu.prove(self.oc, cpu.ProvingKey.parse(self.curve_id, raw), self.zb, *rnd3)[0]
            return formats.proof_raw(self.curve, ref.g16_prove(self.cs, formats.ark_pk_deserialize(self.curve, bytes(raw)), self.z, *rnd3))
        assert self.curve_id < 2
        return cpu.gm17_prove(self.oc, cpu.Gm17ProvingKey.parse(self.curve_id, raw), self.zb, *rnd3)[0]


RND = {"g16": [(0x1234567, 0x89abcdef0123), (0, 7), (1 << 200, 0)], "gm17": [(21, 22, 23), (0, 5, 1 << 199), (7, 0, 0)]}
# one setting at a time against the defaults; msm_c is set before the key is loaded (its tables take the width)
SETTINGS = [{"msm_c": 17}, {"skip_inf": 1}, {"skip_inf": 2}, {"b_sort": 1}, {"b_sort": 2}, {"fuse_z": 0}, {"msm_min_slice": 1}]
DEFAULTS = {"msm_c": 0, "skip_inf": 0, "b_sort": 0, "fuse_z": 1, "msm_min_slice": 8}


def every_entry_point(c, curve_id, scheme, ncs, zb, raw, want, members=3):
    """Lone, resident, resident batch of three and batch from host memory over the key as loaded and bound; the key image; three
    shards and the combination; then one setting at a time.  `want`: the reference's proofs for RND[scheme]."""
    rnds = RND[scheme]
    g = scheme == "g16"
    prove = native.prove_g16 if g else native.prove_gm17
    load = lambda **kw: native.ProvingKey(c, curve_id, raw, scheme=scheme, **kw)

    def lone_and_bound(tag):
        pk = load()
        assert prove(c, pk, ncs, zb, *rnds[0]) == want[0], tag
        pk.bind(ncs)
        assert pk.is_bound(ncs) and prove(c, pk, ncs, zb, *rnds[1]) == want[1], tag
        pk.close()

    pk = load()
    for bound in (False, True):
        if bound:
            pk.bind(ncs)
            assert pk.is_bound(ncs)
        assert [prove(c, pk, ncs, zb, *t) for t in rnds] == want, bound
        za = native.Assignment(c, ncs, zb)
        if g:
            assert native.prove_g16_resident(c, pk, ncs, za, *rnds[1]) == want[1], bound
            assert native.prove_g16_resident_batch(c, pk, ncs, [za] * 3, rnds)[0] == want, bound
            assert native.prove_g16_batch(c, pk, ncs, np.concatenate([zb] * 3), rnds)[0] == want, bound
        else:
            assert native.prove_gm17(c, pk, ncs, za, *rnds[1]) == want[1], bound
            assert native.prove_gm17_resident_batch(c, pk, ncs, [za] * 3, rnds)[0] == want, bound
        za.close()
    pk2 = native.ProvingKey.from_image(c, curve_id, pk.export_image(), scheme=scheme)      # (the image of the bound key)
    assert prove(c, pk2, ncs, zb, *rnds[2]) == want[2]
    pk2.close()
    pk.close()
    shards = [load(rank=k, world=members) for k in range(members)]
    partial, combine = (native.prove_g16_partial, native.combine_g16) if g else (native.prove_gm17_partial, native.combine_gm17)
    parts = [partial(c, shards[k], ncs, zb, *rnds[0]) for k in range(members)]
    assert combine(c, shards[0], parts, *rnds[0]) == want[0]
    for k in shards:
        k.close()
    try:
        for st in SETTINGS:
            for k, v in st.items():
                c.tune(k, v)
            lone_and_bound(st)
            for k in st:
                c.tune(k, DEFAULTS[k])
    finally:
        for k, v in DEFAULTS.items():
            c.tune(k, v)


def twins_everywhere(c, curve_id, scheme, nfill, algorithmic=True):
    curve = CURVES[curve_id]
    cs, z, groups = twin_system(curve, random.Random(0x7717 + 8 * curve_id + nfill), nfill)
    mats = [csr(cs.A), csr(cs.B), csr(cs.C)]
    ncs = native.ConstraintSystem(c, curve_id, cs.n, cs.l, cs.w, mats)
    refs = Refs(curve_id, cs, z, mats, scheme, 0x7E5)
    raw = (native.setup_g16 if scheme == "g16" else native.setup_gm17)(c, ncs, refs.toxic())
    assert raw.tobytes() == refs.key(), "device setup differs from the reference's key"
    check_key_entries(curve_id, scheme, raw, cs, groups)
    want = [refs.closed_form(t) for t in RND[scheme]]
    if algorithmic:
        assert refs.algorithmic(raw, RND[scheme][0]) == want[0]
    every_entry_point(c, curve_id, scheme, ncs, refs.zb, raw, want)
    return cs, z, ncs, refs, raw


PROVERS = [(0, "g16"), (1, "g16"), (0, "gm17")]
_pid = lambda v: "%s-%s" % (CURVES[v[0]].name, v[1])


def test_twin_system_builder():
    """Without any library: satisfied, every kind of group present, members of a group only in their one row."""
    cs, z, groups = twin_system(BN254, random.Random(5), 30)
    assert cs.l == 4 and 50 <= cs.n <= 70
    for kind, xs, sg in groups:
        assert len({z[x] for x in xs}) == 1
        for M in (cs.A, cs.B, cs.C):
            assert sum(1 for row in M if any(j in xs for j, _ in row)) <= 1, kind


@pytest.mark.parametrize("prover", PROVERS, ids=_pid)
def test_proofs_over_twin_variables(ctx, prover):
    twins_everywhere(ctx, *prover, nfill=30)


def test_proofs_over_twin_variables_bls12_377(ctx):
    twins_everywhere(ctx, 2, "g16", nfill=4)


@pytest.mark.gpu
@pytest.mark.parametrize("nfill", [350, 3000])
@pytest.mark.parametrize("prover", PROVERS, ids=_pid)
def test_gpu_proofs_over_twin_variables(gpu_ctx, prover, nfill):
    twins_everywhere(gpu_ctx, *prover, nfill=nfill)


@pytest.mark.gpu
def test_gpu_proofs_over_twin_variables_bls12_377(gpu_ctx):
    twins_everywhere(gpu_ctx, 2, "g16", nfill=4)


# ------------------------------------------------------------------ a key whose entries no honest setup produces
def gm17_pk_deserialize(curve, data):
    """The inverse of oracle.gm17.pk_serialize."""
    rd = formats._Rd(bytes(data))
    g1, g2 = (lambda: formats.de_g1(curve, rd)), (lambda: formats.de_g2(curve, rd))
    vk = dict(h_g2=g2(), g_alpha_g1=g1(), h_beta_g2=g2(), g_gamma_g1=g1(), h_gamma_g2=g2())
    vk["query"] = formats.de_vec(rd, g1)
    pk = dict(vk=vk, a_query=formats.de_vec(rd, g1), b_query=formats.de_vec(rd, g2), c_query_1=formats.de_vec(rd, g1), c_query_2=formats.de_vec(rd, g1))
    pk.update(g_gamma_z=g1(), h_gamma_z=g2(), g_ab_gamma_z=g1(), g_gamma2_z2=g1())
    pk["g_gamma2_z_t"] = formats.de_vec(rd, g1)
    assert rd.o == len(data)
    return pk


def rewritten_key(curve_id, scheme, raw, groups, z, h_bases=True):
    """The honest key `raw` with entries no setup produces.  The bases that pair with h's coefficients (h_query; GM17: the powers
    g_gamma2_z_t; `h_bases`) get a run of equal entries, alternating opposite ones, infinities and an opposite pair; of two groups of
    twins one keeps its equal entries in G1 and loses them in G2, the other the reverse."""
    curve = CURVES[curve_id]
    G1, G2 = group_of(curve_id, 1), group_of(curve_id, 2)
    g = scheme == "g16"
    pk = formats.ark_pk_deserialize(curve, bytes(raw)) if g else gm17_pk_deserialize(curve, bytes(raw))
    h = pk["h_query" if g else "g_gamma2_z_t"]
    assert len(h) >= 48 and all(P is not None for P in h)
    if h_bases:
        h[0:20] = [h[0]] * 20
        h[20:30] = [h[20] if i % 2 == 0 else G1.aneg(h[20]) for i in range(10)]
        h[30] = h[31] = h[len(h) - 1] = None
        h[41] = G1.aneg(h[40])
    twins = [xs for kind, xs, _ in groups if kind == "twins" and z[xs[0]] > 1]      # (a witness value that makes the entry count)
    (x1, x2), (y1, y2) = twins[0], twins[1]
    in_g1, in_g2 = (("a_query", "b_g1_query"), ("b_g2_query",)) if g else (("a_query", "c_query_2") if h_bases else ("a_query",), ("b_query",))
    assert all(pk[q][x1] == pk[q][x2] and pk[q][y1] == pk[q][y2] and pk[q][x1] is not None for q in in_g1 + in_g2)
    for q in in_g2:                              # x1, x2: equal in G1, not in G2
        pk[q][x2] = pk[q][y1]
    for q in in_g1:                              # y1, y2: equal in G2, not in G1
        pk[q][y2] = pk[q][x1]
    out = formats.ark_pk_serialize(curve, pk) if g else ogm17.pk_serialize(curve, pk)
    assert len(out) == len(raw) and out != bytes(raw)
    return np.frombuffer(out, dtype=np.uint8)


def rewritten_key_checks(c, curve_id, scheme, nfill):
    """Unbound, the proof is the algorithmic prover's over the same bytes.  Bound too: the maps the binding applies to h's bases are
    linear in the bases, whatever they are.

    GM17: ark's prover folds 2 d1 U + d1^2 Z - d2 into the quotient, whose coefficients pair with g_gamma2_z_t; the device takes those
    terms from c_query_2 and g_gamma2_z2 (gm17.cuh: the proof depends on d1 and r through rho = r + d1 only), which are the same
    group elements over an honest key only.  Over a key whose a_query and b_query alone are rewritten the two agree for every
    randomness.  Over one whose g_gamma2_z_t and c_query_2 are rewritten as well, what the device computes for (d1, d2, r) is pinned
    as ark's proof over the same bytes for (0, d2, r + d1) — ark's own for d1 = 0 — and for d1 != 0 it is asserted to differ from
    ark's for (d1, d2, r): a key no setup produces has no proof that verifies either way, and the restructuring is the prover's
    design, not something a load could test without pairings."""
    curve = CURVES[curve_id]
    cs, z, groups = twin_system(curve, random.Random(0x7717 + 8 * curve_id + nfill), nfill)
    mats = [csr(cs.A), csr(cs.B), csr(cs.C)]
    ncs = native.ConstraintSystem(c, curve_id, cs.n, cs.l, cs.w, mats)
    refs = Refs(curve_id, cs, z, mats, scheme, 0x7E5)
    raw = np.frombuffer(refs.key(), dtype=np.uint8)
    prove = native.prove_g16 if scheme == "g16" else native.prove_gm17
    rho_form = lambda t: (0, t[1], (t[2] + t[0]) % curve.r)
    variants = [(True, RND["g16"][:2], None)] if scheme == "g16" else [(False, RND["gm17"][:2], None), (True, RND["gm17"], rho_form)]
    for h_bases, rnds, form in variants:
        raw2 = rewritten_key(curve_id, scheme, raw, groups, z, h_bases)
        want = [refs.algorithmic(raw2, form(t) if form else t) for t in rnds]
        assert want[0] != refs.algorithmic(raw, form(rnds[0]) if form else rnds[0]), "the rewritten entries take part in the proof"
        if form:
            arks = [refs.algorithmic(raw2, t) for t in rnds]
            assert [w == a for w, a in zip(want, arks)] == [t[0] == 0 for t in rnds], "ark's own proof where d1 = 0, another where not"
        pk = native.ProvingKey(c, curve_id, raw2, scheme=scheme)
        assert [prove(c, pk, ncs, refs.zb, *t) for t in rnds] == want, ("unbound", h_bases)
        pk.bind(ncs)
        assert pk.is_bound(ncs)
        assert [prove(c, pk, ncs, refs.zb, *t) for t in rnds] == want, ("bound", h_bases)
        pk.close()


@pytest.mark.parametrize("prover", PROVERS + [(2, "g16")], ids=_pid)
def test_rewritten_key(ctx, prover):
    rewritten_key_checks(ctx, *prover, nfill=30 if prover[0] < 2 else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("prover", PROVERS + [(2, "g16")], ids=_pid)
def test_gpu_rewritten_key(gpu_ctx, prover):
    rewritten_key_checks(gpu_ctx, *prover, nfill=350 if prover[0] < 2 else 4)
