"""The witness map's sparse mat-vec (`k_matvec`, K1) at every lane-group width, against the oracle, bit for bit.

`k_matvec` shares a row between G consecutive work-items and joins the G partial sums in an LDS tree; `matvec_group` picks G per
matrix from the average length of the matrix's rows of at most 32 terms, one grid serves the three matrices (sized by the widest;
the workgroups of a narrower matrix that lie past its end leave early).  The chain circuits, the random systems and the compiled
circuits of the other tests all run at G = 1 (Poseidon: B at 2).  The systems here are built from per-matrix lists of row lengths
so that every matrix meets every width 1, 2, 4, 8, 16, in mixes where each matrix is at least once narrower than the launch's
widest, next to an empty row, a one-term row, rows of 31 / 32 / 33 terms side by side and a row of 513 terms (`k_matvec_long`,
`k_matvec_huge`; the short-row kernel skips them inside a shared group).

Every case first asks the library which widths it launches (`ConstraintSystem.matvec_shape`, `zkhip_r1cs_matvec_shape`) and
asserts the ones the generator aimed for: a change of the heuristic fails these tests instead of quietly turning them into
G = 1 tests.

What is compared (no tolerance anywhere): the witness map against the oracle's; `zkhip_r1cs_check` on the satisfied assignment
and on three corrupted ones against <A_i, z> <B_i, z> - <C_i, z> mod r in big integers here; Groth16 (unbound: three matrices,
bound: two, checked over the bound key: three with the check in between), GM17 (`k_sap_rows` reads what the mat-vec left) and
the one-matrix launch of a split proof's second half against the oracle's proofs; and the column sums of the binding at 15 / 16
/ 17 entries and with equal and opposite products.

Both halves: the emulator (`-m "not gpu"`, N = 64: one workgroup holds everything) and the device (`-m gpu`, n = 700, 509, 1: up
to 64 workgroups at width 16 beside 4 at width 1)."""
import random

import numpy as np
import pytest

from oracle import cpu, formats
from oracle import gm17 as ogm17
from oracle import groth16 as g16
from oracle.fields import BN254, BLS12_381
from zokrates_amd import native

GPU = pytest.mark.gpu
NONE = (None, 0)
LONG, HUGE = 32, 512                                   # k_matvec's MATVEC_LONG, k_matvec_huge's MATVEC_HUGE
BANDS = {1: (0, 3), 2: (4, 7), 4: (8, 15), 8: (16, 31), 16: (32, 32)}      # width: sum(short lengths) // n
UNIFORM = [(g, g, g) for g in (1, 2, 4, 8, 16)]
ROTATING = [(1, 4, 16), (16, 1, 4), (4, 16, 1)]
MIXES = UNIFORM + ROTATING + [(2, 8, 2), (8, 2, 16), (16, 16, 1), (1, 16, 16)]
PROVING_ON_EMU = ROTATING + [(16, 16, 16)]
SPLIT_B = (2, 8, 16)                                   # the mixes whose B has one of these widths take the one-matrix launch too
L = 3
THREADS = 4                                            # of the oracle: systems this small lose more to starting a thread per core than to the work


def curve_of(curve_id):
    if curve_id == 2:
        import bls377_ref
        return bls377_ref.CURVE
    return (BN254, BLS12_381)[curve_id]


def le(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8)


def csr(rows):
    """CSR of rows of (column, coefficient) in the order given: duplicates stay what they are."""
    rp, col, val = [0], [], []
    for row in rows:
        for j, v in row:
            col.append(j); val.append(v)
        rp.append(len(col))
    return np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), le(val) if val else np.zeros(0, dtype=np.uint8)


# ------------------------------------------------------------------ the generator
def width_of(lengths):
    """The width the band table gives a matrix with these row lengths."""
    avg = sum(x for x in lengths if x <= LONG) // len(lengths)
    return next(g for g, (lo, hi) in BANDS.items() if lo <= avg <= hi)


def shape_of(lists):
    """What `matvec_shape` has to answer for three lists of row lengths."""
    every = [x for lengths in lists for x in lengths]
    return tuple(width_of(lengths) for lengths in lists), sum(LONG < x <= HUGE for x in every), sum(x > HUGE for x in every)


SPECIAL = ([0, 1, 31, 32, 33, 513], [0, 1, 31, 32, 33, 513], [0, 513, 33, 32, 31, 1])     # A, B, C
START = (2, 11, 2)             # where the block sits: C's empty row on A's (0 * b = 0), B's block elsewhere
TARGET = {1: 3, 2: 6, 4: 12, 8: 24}                    # the average aimed for, + 1/2: the middle of the band (band 0-3: its upper half)
ALONE = {1: 3, 2: 5, 4: 9, 8: 17, 16: 32}              # n = 1: the one row's length is the average


def row_lengths(rnd, n, width, which):
    """n row lengths of matrix `which` (0: A, 1: B, 2: C) whose short rows average into the band of `width`."""
    if width == 16:
        return [32] * n                                # the only way to an average of 32
    if n == 1:
        return [ALONE[width]]
    assert n >= 30
    k = n - len(SPECIAL[which])
    total = TARGET[width] * n + n // 2 - sum(x for x in SPECIAL[which] if x <= LONG)
    fill = [total // k + 1] * (total % k) + [total // k] * (k - total % k)
    least = 1 if which == 2 else 0                     # (an empty row of C needs a = 0 or b = 0: the block's one is placed for that)
    for _ in range(2 * k):                             # the same sum, spread
        i, j = rnd.randrange(k), rnd.randrange(k)
        d = rnd.randrange(0, min(fill[i] - least, LONG - fill[j], 5) + 1) if i != j else 0
        fill[i] -= d; fill[j] += d
    rnd.shuffle(fill)
    out = fill[:START[which]] + SPECIAL[which] + fill[START[which]:]
    assert len(out) == n and all(0 <= x <= LONG for x in fill)
    return out


class System:
    """A satisfied R1CS from three lists of row lengths.  z first (z_0 = 1, the others random and non-zero); A and B rows random;
    each non-empty C row has its last coefficient solved for; under an empty C row a coefficient of A (or B) is solved so that the
    row's product is 0.  Coefficients from {1, r - 1, below 2^40, full width}."""

    def __init__(self, curve_id, lists, seed, l=L):
        self.curve_id, self.curve, self.l = curve_id, curve_of(curve_id), l
        r = self.r = self.curve.r
        rnd = self.rnd = random.Random(seed)
        self.lists = lists
        self.n = len(lists[0])
        self.m = max(40, max(max(x) for x in lists) + 8)
        self.w = self.m - l
        self.z = [1] + [rnd.randrange(1, r) for _ in range(self.m - 1)]
        coef = lambda: (lambda: 1, lambda: r - 1, lambda: rnd.randrange(1, 1 << 40), lambda: rnd.randrange(1, r))[rnd.randrange(4)]()
        lc = lambda length: [(c, coef()) for c in rnd.sample(range(self.m), length)]

        def solve(row, value):                         # the last coefficient of `row` so that <row, z> = value
            j = row[-1][0]
            row[-1] = (j, (value - self.dot(row[:-1], self.z)) * pow(self.z[j], r - 2, r) % r)

        self.A, self.B, self.C = [], [], []
        for i in range(self.n):
            a, b, c = lc(lists[0][i]), lc(lists[1][i]), lc(lists[2][i])
            if c:
                solve(c, self.dot(a, self.z) * self.dot(b, self.z) % r)
            elif a and b:
                solve(a if len(a) >= 2 else b, 0)
                assert len(a) >= 2 or len(b) >= 2
            self.A.append(a); self.B.append(b); self.C.append(c)
        self.finish()

    def finish(self):
        self.mats = [csr(M) for M in (self.A, self.B, self.C)]
        self.zb = le(self.z)
        assert self.failing(self.z) == []
        for M, lengths in zip((self.A, self.B, self.C), self.lists):
            assert [len(row) for row in M] == lengths
        self.shape = shape_of(self.lists)

    def dot(self, row, z):
        return sum(v * z[j] for j, v in row) % self.r

    def failing(self, z):
        """The reference of `zkhip_r1cs_check`: the rows with <A_i, z> <B_i, z> - <C_i, z> != 0 mod r."""
        return [i for i in range(self.n) if (self.dot(self.A[i], z) * self.dot(self.B[i], z) - self.dot(self.C[i], z)) % self.r]

    def column_in_a_row_of(self, lo, hi):
        """A column (not ONE) of the first row, over A, B, C, with lo <= terms <= hi; None if there is no such row."""
        for M in (self.A, self.B, self.C):
            for row in M:
                if lo <= len(row) <= hi:
                    cols = [j for j, _ in row if j != 0]
                    if cols:
                        return cols[len(cols) // 2]
        return None

    def corrupted(self):
        """Three copies of z with one variable changed each: one of a short row, one of a 33-term row, one of the 513-term row
        (systems without such rows, width 16 throughout or n = 1, take further short rows' variables)."""
        picks = [self.column_in_a_row_of(1, LONG), self.column_in_a_row_of(33, 33), self.column_in_a_row_of(513, 513)]
        spare = list(dict.fromkeys(j for M in (self.C, self.B, self.A) for row in M if len(row) <= LONG for j, _ in row if j != 0 and j not in picks))
        out = []
        for j in picks:
            j = spare.pop() if j is None else j
            z = list(self.z)
            z[j] = (z[j] + 1) % self.r
            out.append(z)
        return out

    def load(self, ctx):
        dcs = native.ConstraintSystem(ctx, self.curve_id, self.n, self.l, self.w, self.mats)
        assert dcs.matvec_shape() == self.shape        # the widths that run are the ones aimed for
        assert max(dcs.matvec_shape()[0]) <= 16
        return dcs

    def oracle_circuit(self):
        return cpu.Circuit.from_csr(self.curve_id, self.n, self.l, self.w, self.mats)

    def oracle_r1cs(self):
        cs = g16.R1CS(l=self.l, w=self.w)
        cs.A, cs.B, cs.C = self.A, self.B, self.C
        return cs


_systems = {}


def mixed(curve_id, n, mix):
    """The system of a case: built once, shared by the tests that use it, left unchanged."""
    key = (curve_id, n, mix)
    if key not in _systems:
        rnd = random.Random("lengths %d %d %s" % (curve_id, n, mix))
        lists = [row_lengths(rnd, n, mix[k], k) for k in range(3)]
        _systems[key] = System(curve_id, lists, "system %d %d %s" % key)
        assert _systems[key].shape[0] == mix
        if n > 1:                                      # the rows the docstring names are there, the long ones in every narrow matrix
            narrow = sum(g < 16 for g in mix)
            assert _systems[key].shape[1:] == (narrow, narrow)
            for k in range(3):
                if mix[k] < 16:                        # (31 | 32 | 33 side by side inside the block)
                    assert lists[k][START[k]:START[k] + len(SPECIAL[k])] == SPECIAL[k]
    return _systems[key]


# ------------------------------------------------------------------ contexts
_contexts = {}


@pytest.fixture(scope="module")
def contexts():
    yield _contexts
    for c in _contexts.values():
        c.close()
    _contexts.clear()
    _systems.clear()


def context(contexts, backend, rank=None):
    """The context of a backend; `rank` 0 / 1: two more of its kind, the ranks of a split proof."""
    key = backend if rank is None else "%s rank %d" % (backend, rank)
    if key not in contexts:
        if backend == "gpu":
            contexts[key] = native.Context(0)
            assert "gfx950" in contexts[key].describe()
        else:
            from emu_util import emu_library
            contexts[key] = native.Context(0, emu_library())
            assert "EMULATOR" in contexts[key].describe()
    return contexts[key]


def ident(v):
    return "x".join(str(g) for g in v) if isinstance(v, tuple) else str(v)


def cases(emu_sizes, gpu_sizes, emu_mixes=MIXES, gpu_mixes=MIXES, third_curve=ROTATING):
    out = []
    for backend, sizes, mixes in (("emu", emu_sizes, emu_mixes), ("gpu", gpu_sizes, gpu_mixes)):
        for curve_id in (0, 1, 2) if backend == "gpu" else (0, 1):
            for n in sizes:
                for mix in mixes:
                    if curve_id < 2 or mix in third_curve:
                        out.append(pytest.param(backend, curve_id, n, mix, marks=[GPU] if backend == "gpu" else [],
                                                id="-".join(ident(v) for v in (backend, curve_id, n, mix))))
    return out


# ------------------------------------------------------------------ 1, 2: the witness map and the check, every mix
@pytest.mark.parametrize("backend,curve_id,n,mix", cases((61, 30), (700, 509, 1)))
def test_witness_map_and_check(contexts, backend, curve_id, n, mix):
    """n + l = N exactly (61, 509: no zero-filled tail); half the domain a zero-filled tail (30); N = 1024 with 64 workgroups at width
    16 beside 4 at width 1 (700); far less than one workgroup's rows (1)."""
    ctx = context(contexts, backend)
    sy = mixed(curve_id, n, mix)
    dcs = sy.load(ctx)
    if curve_id == 2:
        want = le(g16.witness_map(sy.curve, sy.oracle_r1cs(), sy.z))
    else:
        want = cpu.witness_map(sy.oracle_circuit(), sy.zb, THREADS)
    assert dcs.witness_map(sy.zb).tobytes() == want.tobytes()
    assert dcs.check(sy.zb) == NONE
    for z in sy.corrupted():
        bad = sy.failing(z)
        assert bad, "the corrupted variable is in a row"
        assert dcs.check(le(z)) == (bad[0], len(bad))
    assert dcs.check(sy.zb) == NONE
    dcs.close()


# ------------------------------------------------------------------ 3, 4, 5: proofs
def g16_want(sy, tox, r_, s_, raw):
    """The oracle's Groth16 proof (closed form), the algorithmic prover's agreeing with it, the key's bytes the oracle's own."""
    if sy.curve_id == 2:
        import bls377_ref as ref
        cs = sy.oracle_r1cs()
        want = formats.proof_raw(sy.curve, ref.g16_trapdoor(cs, tox, sy.z, r_, s_))
        if sy.m <= 40:                                 # (the Python set-up of a 521-variable key takes several seconds)
            opk, _ = ref.g16_setup(cs, tox)
            assert raw.tobytes() == formats.ark_pk_serialize(sy.curve, opk)
            assert formats.proof_raw(sy.curve, ref.g16_prove(cs, opk, sy.z, r_, s_)) == want
        return want
    oc, tb = sy.oracle_circuit(), cpu.toxic_bytes(tox)
    assert raw.tobytes() == cpu.ProvingKey.setup(oc, tb, THREADS).serialize().tobytes()
    want = cpu.trapdoor(oc, tb, sy.zb, r_, s_, THREADS)
    assert cpu.prove(oc, cpu.ProvingKey.parse(sy.curve_id, raw), sy.zb, r_, s_, THREADS)[0] == want
    return want


def gm17_want(sy, tox, d1, d2, r_, raw):
    if sy.curve_id == 2:
        import bls377_ref as ref
        cs = sy.oracle_r1cs()
        want = formats.proof_raw(sy.curve, ref.gm17_trapdoor(cs, tox, sy.z, d1, r_))
        if sy.m <= 40:
            opk, _ = ref.gm17_setup(cs, tox)
            assert raw.tobytes() == ogm17.pk_serialize(sy.curve, opk)
            assert formats.proof_raw(sy.curve, ref.gm17_prove(cs, opk, sy.z, d1, d2, r_)) == want
        return want
    oc, tb = sy.oracle_circuit(), cpu.gm17_toxic_bytes(tox)
    opk = cpu.Gm17ProvingKey.setup(oc, tb, THREADS)
    assert raw.tobytes() == opk.serialize().tobytes()
    want = cpu.gm17_trapdoor(oc, tb, sy.zb, d1, r_, THREADS)
    assert cpu.gm17_prove(oc, opk, sy.zb, d1, d2, r_, THREADS)[0] == want
    return want


def groth16_everywhere(ctx, sy, dcs):
    """Unbound (A, B, C in one launch), bound (A and B), checked over the bound key (three again, the check in between)."""
    tox = g16.Toxic.from_seed(sy.curve, 0x517 + sy.n)
    raw = native.setup_g16(ctx, dcs, (tox.alpha, tox.beta, tox.gamma, tox.delta, tox.tau))
    r_, s_ = sy.rnd.randrange(sy.r), sy.rnd.randrange(sy.r)
    want = g16_want(sy, tox, r_, s_, raw)
    pk = native.ProvingKey(ctx, sy.curve_id, raw)
    try:
        assert native.prove_g16(ctx, pk, dcs, sy.zb, r_, s_) == want
        pk.bind(dcs)
        assert pk.is_bound(dcs)
        assert native.prove_g16(ctx, pk, dcs, sy.zb, r_, s_) == want
        ctx.set_checked(True)
        assert native.prove_g16(ctx, pk, dcs, sy.zb, r_, s_) == want
    finally:
        ctx.set_checked(False)
        pk.close()
    return raw, want, (r_, s_)


def split_proof(contexts, backend, sy, raw, r_, s_):
    """Two ranks, each with a shard bound to the system: rank 1 transforms b alone (`mat0 = 1`: the launch runs B at its own
    width, A and C count as 1)."""
    ranks = []
    for k in range(2):
        c = context(contexts, backend, k)
        cs = sy.load(c)
        sh = native.ProvingKey(c, sy.curve_id, raw, rank=k, world=2)
        sh.bind_shard(cs, raw)
        ranks.append((c, cs, sh))
    halves = [native.prove_g16_split_begin(c, sh, cs, sy.zb, r_, s_, k) for k, (c, cs, sh) in enumerate(ranks)]
    parts = [native.prove_g16_split_end(c, sh, cs, halves[1 - k]) for k, (c, cs, sh) in enumerate(ranks)]
    proof = native.combine_g16(ranks[0][0], ranks[0][2], parts, r_, s_)
    for c, cs, sh in ranks:
        sh.close(); cs.close()
    return proof


@pytest.mark.parametrize("backend,curve_id,n,mix", cases((30,), (700, 509, 1), emu_mixes=PROVING_ON_EMU))
def test_groth16_unbound_bound_checked_and_split(contexts, backend, curve_id, n, mix):
    ctx = context(contexts, backend)
    sy = mixed(curve_id, n, mix)
    dcs = sy.load(ctx)
    raw, want, (r_, s_) = groth16_everywhere(ctx, sy, dcs)
    if mix[1] in SPLIT_B and curve_id < 2:
        assert split_proof(contexts, backend, sy, raw, r_, s_) == want
    dcs.close()


@pytest.mark.parametrize("backend,curve_id,n,mix", cases((30,), (), emu_mixes=[(2, 8, 2), (8, 2, 16)]))
def test_split_proof_with_b_at_2_and_8_on_emulator(contexts, backend, curve_id, n, mix):
    """The one-matrix launch with B at 2 and at 8 lanes (the proving mixes of the emulator half have B at 4, 1, 16, 16)."""
    ctx = context(contexts, backend)
    sy = mixed(curve_id, n, mix)
    dcs = sy.load(ctx)
    tox = g16.Toxic.from_seed(sy.curve, 0x517 + sy.n)
    raw = native.setup_g16(ctx, dcs, (tox.alpha, tox.beta, tox.gamma, tox.delta, tox.tau))
    assert split_proof(contexts, backend, sy, raw, 71, 72) == cpu.trapdoor(sy.oracle_circuit(), cpu.toxic_bytes(tox), sy.zb, 71, 72, THREADS)
    dcs.close()


@pytest.mark.parametrize("backend,curve_id,n,mix", cases((30,), (700, 509, 1), emu_mixes=PROVING_ON_EMU))
def test_gm17(contexts, backend, curve_id, n, mix):
    ctx = context(contexts, backend)
    sy = mixed(curve_id, n, mix)
    dcs = sy.load(ctx)
    tox = ogm17.Toxic.from_seed(sy.curve, 0x717 + sy.n)
    raw = native.setup_gm17(ctx, dcs, (tox.alpha, tox.beta, tox.gamma, tox.t))
    d1, d2, r_ = (sy.rnd.randrange(sy.r) for _ in range(3))
    want = gm17_want(sy, tox, d1, d2, r_, raw)
    pk = native.ProvingKey(ctx, sy.curve_id, raw, scheme="gm17")
    assert native.prove_gm17(ctx, pk, dcs, sy.zb, d1, d2, r_) == want
    pk.close()
    dcs.close()


# ------------------------------------------------------------------ the binding's column sums
def column_system(curve_id, n, counts):
    """A and B of mix (2, 8, 2); C laid out by column.  Returns the system and {what: column}."""
    rnd = random.Random("columns %d %d" % (curve_id, n))
    lists = [row_lengths(rnd, n, g, k) for k, g in enumerate((2, 8, 2))]
    sy = System(curve_id, lists, "column system %d %d" % (curve_id, n))
    r, m = sy.r, sy.m
    coef = lambda: rnd.choice([1, r - 1, rnd.randrange(1, 1 << 40), rnd.randrange(1, r)])
    C = [[] for _ in range(n)]
    named = {}
    first = sy.l + 2
    for q, count in enumerate(counts):                 # witness variables with exactly `count` entries, in rows of their own choice
        named[count] = first + q
        for i in rnd.sample(range(n), count):
            C[i].append((first + q, coef()))
    v = first + len(counts)
    named["equal"], named["opposite"], named["public"], named["last"] = v, v + 1, 1, m - 1
    same, h = coef(), rnd.randrange(1, r)
    C[n // 3] += [(v, same), (v, same)]                # the same product twice: the sum's addition meets a doubling
    C[n // 2] += [(v + 1, h), (v + 1, r - h), (v + 1, coef())]      # h P + (r - h) P: the point at infinity on the way
    for i in rnd.sample(range(n), 17):
        C[i].append((1, coef()))
    solvers = list(range(v + 2, m - 1))                # every row ends in a solved coefficient on one of the other variables
    for i in range(n):
        rnd.shuffle(C[i])
        C[i].append((rnd.choice(solvers), 0))
        j = C[i][-1][0]
        C[i][-1] = (j, (sy.dot(sy.A[i], sy.z) * sy.dot(sy.B[i], sy.z) - sy.dot(C[i][:-1], sy.z)) * pow(sy.z[j], r - 2, r) % r)
    sy.C = C
    sy.lists = [lists[0], lists[1], [len(row) for row in C]]
    sy.finish()
    return sy, named


@pytest.mark.parametrize("backend,curve_id", [pytest.param(b, c, marks=[GPU] if b == "gpu" else [], id="%s-%d" % (b, c))
                                              for b in ("emu", "gpu") for c in (0, 1)])
def test_binding_columns_around_the_short_column_bound(contexts, backend, curve_id):
    """`k_bind_l_sum_short` sums the columns of at most BIND_SHORT_COL = 16 entries, `_long` the others: columns of 0, 1, 15, 16,
    17 and more entries, a column whose two products are equal, one whose first two cancel, a public variable's column of 17, the
    last variable with none.  The unbound proof, the bound proof and the oracle's closed form are the same bytes."""
    ctx = context(contexts, backend)
    n, counts = (700, [0, 1, 15, 16, 17, 63, 64, 65, 200]) if backend == "gpu" else (61, [0, 1, 15, 16, 17, 40])
    sy, named = column_system(curve_id, n, counts)
    have = np.bincount(sy.mats[2][1], minlength=sy.m)            # the columns' lengths, counted from the CSR
    for count in counts:
        assert have[named[count]] == count
    assert have[named["equal"]] == 2 and have[named["opposite"]] == 3 and have[named["public"]] == 17 and have[named["last"]] == 0
    assert sy.shape[0][:2] == (2, 8)
    dcs = sy.load(ctx)
    tox = g16.Toxic.from_seed(sy.curve, 0xC01)
    tb, oc = cpu.toxic_bytes(tox), sy.oracle_circuit()
    raw = native.setup_g16(ctx, dcs, (tox.alpha, tox.beta, tox.gamma, tox.delta, tox.tau))
    assert raw.tobytes() == cpu.ProvingKey.setup(oc, tb, THREADS).serialize().tobytes()
    want = cpu.trapdoor(oc, tb, sy.zb, 51, 52, THREADS)
    pk = native.ProvingKey(ctx, curve_id, raw)
    unbound = native.prove_g16(ctx, pk, dcs, sy.zb, 51, 52)
    pk.bind(dcs)
    assert pk.is_bound(dcs)
    bound = native.prove_g16(ctx, pk, dcs, sy.zb, 51, 52)
    assert unbound == want and bound == want
    assert dcs.witness_map(sy.zb).tobytes() == cpu.witness_map(oc, sy.zb, THREADS).tobytes()
    pk.close()
    dcs.close()


# ------------------------------------------------------------------ matvec_shape at its edges (host logic: the emulator)
def shape_from_lists(ctx, lists, m=48):
    rnd = random.Random(5)
    mats = [csr([[(j, 1 + rnd.randrange(9)) for j in rnd.sample(range(m), length)] for length in lengths]) for lengths in lists]
    cs = native.ConstraintSystem(ctx, 0, len(lists[0]), L, m - L, mats)
    shape = cs.matvec_shape()
    cs.close()
    assert shape == shape_of(lists)
    return shape


def test_matvec_shape_edges(contexts):
    ctx = context(contexts, "emu")
    assert shape_from_lists(ctx, [[0] * 7] * 3) == ((1, 1, 1), 0, 0)                        # all-empty matrices
    assert shape_from_lists(ctx, [[32], [0], [31]]) == ((16, 1, 8), 0, 0)                  # n = 1: one row of 32 terms
    assert shape_from_lists(ctx, [[33], [32], [33]]) == ((1, 16, 1), 2, 0)                 # one row of 33 terms: long, and width 1
    assert shape_from_lists(ctx, [[32, 32, 32, 33], [32] * 4, [3, 4, 4, 4]]) == ((8, 16, 1), 1, 0)       # 96 // 4 = 24; 15 // 4 = 3
    assert shape_from_lists(ctx, [[32, 32, 32, 31], [4] * 4, [16] * 4]) == ((8, 2, 8), 0, 0)             # one term short of 16
    assert shape_from_lists(ctx, [[512, 513, 8], [600, 33, 7], [0, 0, 24]], m=640) == ((1, 1, 4), 2, 2)
    # no system of this file asks for more than 16 lanes (System.load asserts it for each as it is loaded): nor does the densest one
    assert shape_from_lists(ctx, [[32] * 40] * 3) == ((16, 16, 16), 0, 0)
    for curve_id, n, mix in [(0, 30, m) for m in MIXES] + [(1, 61, m) for m in MIXES]:
        assert mixed(curve_id, n, mix).shape[0] == mix and max(mixed(curve_id, n, mix).shape[0]) <= 16
