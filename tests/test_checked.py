"""Checked proving: `zkhip_r1cs_check` (Az o Bz == Cz on the device, the lowest failing row and the number of failing rows),
the checked mode of a context (`zkhip_ctx_set_checked`, `zkhip_ctx_unsatisfied`) and `generate-proof --check`.

The reference of every assertion is plain big-integer arithmetic in this file: <A_i, z> * <B_i, z> - <C_i, z> mod r per row
(`failing_rows`), from which the expected first row and count follow exactly — no tolerance anywhere.  The circuits are
assembled by hand as CSR: row k is (u_k + c_k) * (v_k + d_k x) = t_k over variables of its own, so one corrupted witness
value fails exactly the row that mentions it; rows of more than 32 and more than 512 terms take the mat-vec's other kernels.

Every case runs on the emulator (`-m "not gpu"`: bn128 and bls12_381, the curves it is built for) and on the GPU (`-m gpu`:
bls12_377 as well)."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu, ir
from oracle.fields import BN254, BLS12_381
from zokrates_amd import native, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NONE = (None, 0)                       # ConstraintSystem.check of a satisfied system
GPU = pytest.mark.gpu


def on(backend, *values):
    return pytest.param(backend, *values, marks=[GPU] if backend == "gpu" else [], id="-".join([backend] + [str(v) for v in values]))


_contexts = {}


@pytest.fixture(scope="module")
def contexts():
    yield _contexts
    for c in _contexts.values():
        c.close()
    _contexts.clear()


def context(contexts, backend):
    if backend not in contexts:
        if backend == "gpu":
            contexts[backend] = native.Context(0)
            assert "gfx950" in contexts[backend].describe()
        else:
            from emu_util import emu_library
            contexts[backend] = native.Context(0, emu_library())
            assert "EMULATOR" in contexts[backend].describe()
    return contexts[backend]


# ------------------------------------------------------------------ circuits by hand and the big-integer reference
class Rows:
    """An R1CS as Python lists: rows[i] = (A terms, B terms, C terms), a term = (column, value); l = 2 (ONE, x)."""

    def __init__(self, curve_id):
        self.curve_id, self.p = curve_id, synth.FR_MODULUS[curve_id]
        self.rows, self.z = [], [1, 0x1234567 % self.p]
        self.l = 2
        self.rnd = np.random.default_rng(0xC0DE + curve_id)

    def field(self):
        return int.from_bytes(self.rnd.bytes(40), "little") % self.p

    def var(self, value):
        self.z.append(value % self.p)
        return len(self.z) - 1

    def product_row(self):
        """(u + c) * (v + d x) = t over three variables no other row mentions.  Returns (u, v, t)."""
        c, d, uv, vv = (self.field() for _ in range(4))
        u, v = self.var(uv), self.var(vv)
        t = self.var((uv + c) * (vv + d * self.z[1]))
        self.rows.append(([(u, 1), (0, c)], [(v, 1), (1, d)], [(t, 1)]))
        return u, v, t

    def sum_row(self, terms):
        """(sum_j a_j s_j) * ONE = t over `terms` + 1 variables of its own.  Returns (the s columns, t)."""
        coef = [self.field() for _ in range(terms)]
        val = [self.field() for _ in range(terms)]
        s = [self.var(v) for v in val]
        t = self.var(sum(a * v for a, v in zip(coef, val)))
        self.rows.append((list(zip(s, coef)), [(0, 1)], [(t, 1)]))
        return s, t

    @property
    def n(self):
        return len(self.rows)

    @property
    def w(self):
        return len(self.z) - self.l

    def mats(self):
        out = []
        for k in range(3):
            rp = np.zeros(self.n + 1, dtype=np.uint64)
            rp[1:] = np.cumsum([len(r[k]) for r in self.rows])
            col = np.array([c for r in self.rows for c, _ in r[k]], dtype=np.uint32)
            val = np.frombuffer(b"".join((v % self.p).to_bytes(32, "little") for r in self.rows for _, v in r[k]), dtype=np.uint8)
            out.append((rp, col, val))
        return out

    def assignment(self, changed=()):
        """uint8[m * 32]; `changed` = columns whose value gets one added."""
        z = list(self.z)
        for c in changed:
            z[c] = (z[c] + 1) % self.p
        return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in z), dtype=np.uint8), z

    def load(self, ctx):
        return native.ConstraintSystem(ctx, self.curve_id, self.n, self.l, self.w, self.mats())


def failing_rows(rows, z):
    dot = lambda terms: sum(v * z[c] for c, v in terms)
    return [i for i, (a, b, c) in enumerate(rows.rows) if (dot(a) * dot(b) - dot(c)) % rows.p]


def verdict(rows, z):
    bad = failing_rows(rows, z)
    return (bad[0], len(bad)) if bad else NONE


def product_circuit(curve_id, n):
    rows = Rows(curve_id)
    cols = [rows.product_row() for _ in range(n)]
    return rows, cols


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


STANDALONE = [on("emu", 0), on("emu", 1), on("gpu", 0), on("gpu", 1), on("gpu", 2)]


# ------------------------------------------------------------------ the stand-alone check
@pytest.mark.parametrize("backend,curve_id", STANDALONE)
def test_one_failing_row_at_every_boundary(contexts, backend, curve_id):
    """n in {1, 5, 255, 256, 257, 4097}; the one failing row at 0, at n - 1 and on either side of a wavefront (63 | 64) and of a
    workgroup (255 | 256) boundary; a satisfied system says (UINT64_MAX, 0) — `None, 0` here."""
    ctx = context(contexts, backend)
    for n in (1, 5, 255, 256, 257, 4097):
        rows, cols = cached(("product", curve_id, n), lambda: product_circuit(curve_id, n))
        cs = rows.load(ctx)
        zb, z = rows.assignment()
        assert failing_rows(rows, z) == []
        assert cs.check(zb) == NONE, n
        assert cs.check(native.Assignment(ctx, cs, zb)) == NONE, n        # the resident form of the same call
        for k in sorted({0, n - 1} | {r for r in (63, 64, 255, 256) if r < n}):
            for which in (0, 2):                                           # u_k (in A only), t_k (in C only)
                zb, z = rows.assignment([cols[k][which]])
                assert failing_rows(rows, z) == [k]
                assert cs.check(zb) == (k, 1), (n, k, which)
        cs.close()


@pytest.mark.parametrize("backend,curve_id", STANDALONE)
def test_failing_rows_in_different_workgroups(contexts, backend, curve_id):
    """Two and three failing rows far apart: the lowest one, and the exact count."""
    ctx = context(contexts, backend)
    n = 4097
    rows, cols = cached(("product", curve_id, n), lambda: product_circuit(curve_id, n))
    cs = rows.load(ctx)
    for picks in ((3000, 70), (4096, 1500, 300), (256, 255), (4000, 64, 63)):
        zb, z = rows.assignment([cols[k][2] for k in picks])
        assert failing_rows(rows, z) == sorted(picks)
        assert cs.check(zb) == (min(picks), len(picks)), picks
        assert cs.check(native.Assignment(ctx, cs, zb)) == (min(picks), len(picks)), picks
    # every row at once: the public input x is in B of all of them.  The input-consistency rows (n .. n + l - 1 of A) are no
    # constraints and never show: first_row < n
    zb, z = rows.assignment([1])
    want = verdict(rows, z)
    assert want[1] > 4000 and want[0] < n
    assert cs.check(zb) == want
    cs.close()


@pytest.mark.parametrize("backend,curve_id", STANDALONE)
def test_long_and_huge_rows_and_a_variable_only_c_mentions(contexts, backend, curve_id):
    """The failing row is one of more than 32 terms (k_matvec_long), of more than 512 (k_matvec_huge), and one whose corrupted
    variable only C mentions."""

    def make():
        rows = Rows(curve_id)
        cols = [rows.product_row() for _ in range(70)]
        long_s, long_t = rows.sum_row(40)           # row 70
        cols += [rows.product_row() for _ in range(60)]
        huge_s, huge_t = rows.sum_row(600)          # row 131
        cols += [rows.product_row() for _ in range(9)]
        return rows, cols, long_s, long_t, huge_s, huge_t

    rows, cols, long_s, long_t, huge_s, huge_t = cached(("long", curve_id), make)
    ctx = context(contexts, backend)
    cs = rows.load(ctx)
    zb, z = rows.assignment()
    assert failing_rows(rows, z) == [] and cs.check(zb) == NONE
    for changed, want in (([long_s[0]], (70, 1)), ([long_s[39]], (70, 1)), ([long_t], (70, 1)), ([huge_s[0]], (131, 1)), ([huge_s[599]], (131, 1)),
                          ([huge_s[300], long_s[7]], (70, 2)), ([huge_t], (131, 1)), ([cols[135][2]], (137, 1)), ([cols[5][2], huge_t], (5, 2))):
        zb, z = rows.assignment(changed)
        assert verdict(rows, z) == want
        assert cs.check(zb) == want, changed
    # an instance variable (column < l)
    zb, z = rows.assignment([1])
    want = verdict(rows, z)
    assert want[1] >= 130 and want[0] < rows.n
    assert cs.check(zb) == want
    cs.close()


def test_check_refuses_what_the_prover_refuses(contexts):
    """z[0] != 1 and a non-canonical entry are argument errors, as in the prove calls — not verdicts."""
    ctx = context(contexts, "emu")
    rows, cols = cached(("product", 0, 5), lambda: product_circuit(0, 5))
    cs = rows.load(ctx)
    zb, _ = rows.assignment()
    bad = np.array(zb, copy=True)
    bad[0] = 2
    with pytest.raises(native.ZkhipError) as e:
        cs.check(bad)
    assert e.value.code == -1
    bad = np.array(zb, copy=True)
    bad[32 * 3:32 * 4] = 0xff
    with pytest.raises(native.ZkhipError) as e:
        cs.check(bad)
    assert e.value.code == -1
    assert cs.check(zb) == NONE
    assert ctx.set_checked(None) is False           # off by default; reporting changes nothing
    cs.close()


# ------------------------------------------------------------------ checked proving
def proving_case(ctx, backend, scheme, curve_id):
    """A circuit whose domain takes the two-pass transform under the context's NTT_SINGLE_MAX_LOG (emulator: 14 rows, 2^4 / SAP 2^5
    at a limit of 2^1; GPU: 1022 rows, 2^10 / SAP 2^11 at 2^5), its key from the device setup, its system."""
    n = 1022 if backend == "gpu" else 14
    rows, cols = cached(("product", curve_id, n), lambda: product_circuit(curve_id, n))
    cs = rows.load(ctx)
    tox = synth.toxic_waste(curve_id)
    if scheme == "gm17":
        raw = native.setup_gm17(ctx, cs, (tox[0], tox[1], tox[2], tox[4]))
    else:
        raw = native.setup_g16(ctx, cs, tox)
    pk = native.ProvingKey(ctx, curve_id, raw, scheme=scheme)
    return rows, cols, cs, pk, raw


def prove(ctx, scheme, pk, cs, z, rnd):
    if scheme == "gm17":
        return native.prove_gm17(ctx, pk, cs, z, rnd[0], 7, rnd[1])
    return native.prove_g16(ctx, pk, cs, z, *rnd)


def prove_batch(ctx, scheme, pk, cs, zs, rnds):
    if scheme == "gm17":
        return native.prove_gm17_resident_batch(ctx, pk, cs, zs, [(a, 7, b) for a, b in rnds])[0]
    return native.prove_g16_resident_batch(ctx, pk, cs, zs, rnds)[0]


PROVING = [on("emu", "g16", 0), on("emu", "g16", 1), on("emu", "gm17", 0), on("emu", "gm17", 1),
           on("gpu", "g16", 0), on("gpu", "g16", 1), on("gpu", "gm17", 0), on("gpu", "gm17", 2)]
RNDS = [(0x1111 * (i + 1), 0x2222 * (i + 3)) for i in range(4)]


@pytest.fixture
def two_pass(contexts, request):
    """The context of the case's backend with the single-pass limit lowered for the duration of the test."""
    backend = request.node.callspec.params["backend"]
    ctx = context(contexts, backend)
    ctx.tune("ntt_single_max_log", 5 if backend == "gpu" else 1)
    yield ctx
    ctx.set_checked(False)
    ctx.tune("stream_jitter", 0)
    ctx.tune("ntt_single_max_log", 10)


@pytest.mark.parametrize("backend,scheme,curve_id", PROVING)
def test_checked_proving(two_pass, backend, scheme, curve_id):
    ctx = two_pass
    rows, cols, cs, pk, raw = proving_case(ctx, backend, scheme, curve_id)
    bad_row = rows.n - 3
    zg, _ = rows.assignment()
    zb, zbad = rows.assignment([cols[bad_row][2]])             # t of that row: only C mentions it
    assert failing_rows(rows, zbad) == [bad_row]
    zs = [native.Assignment(ctx, cs, z) for z in (zg, zg, zb, zg)]
    for bound in (False, True):
        if bound:
            pk.bind(cs)
            assert pk.is_bound(cs)
        # ---- checked mode off (the default): a bad witness is proof bytes and ZKHIP_OK, as it always was
        assert ctx.set_checked(None) is False
        plain = [prove(ctx, scheme, pk, cs, zg, RNDS[i]) for i in range(4)]
        plain_bad = prove(ctx, scheme, pk, cs, zb, RNDS[2])
        assert plain_bad == prove(ctx, scheme, pk, cs, zb, RNDS[2]) and any(plain_bad) and plain_bad != plain[2]
        if scheme == "g16":                                    # ... the bytes the oracle computes for that unsatisfying assignment
            oc = cpu.Circuit.from_csr(curve_id, rows.n, rows.l, rows.w, rows.mats())
            assert plain_bad == cpu.prove(oc, cpu.ProvingKey.parse(curve_id, raw), zb, *RNDS[2])[0]
        assert prove_batch(ctx, scheme, pk, cs, zs, RNDS) == plain[:2] + [plain_bad] + plain[3:]
        # ---- on: a good witness gives the same bytes through every entry point
        assert ctx.set_checked(True) is False and ctx.set_checked(None) is True
        assert [prove(ctx, scheme, pk, cs, zg, RNDS[i]) for i in range(4)] == plain
        resident = prove(ctx, scheme, pk, cs, zs[0], RNDS[0]) if scheme == "gm17" else native.prove_g16_resident(ctx, pk, cs, zs[0], *RNDS[0])
        assert resident == plain[0]
        assert prove_batch(ctx, scheme, pk, cs, [zs[0]] * 4, RNDS) == plain
        if scheme == "g16":
            assert native.prove_g16_batch(ctx, pk, cs, np.concatenate([zg] * 4), RNDS)[0] == plain
        # ---- a bad one (over the bound key this needs C's mat-vec, which the proof itself does not run)
        with pytest.raises(native.ZkhipError) as e:
            prove(ctx, scheme, pk, cs, zb, RNDS[2])
        assert e.value.code == -5 and e.value.unsatisfied == [(0, bad_row, 1)]
        assert "proof 0 of 1: constraint %d of %d is not satisfied (1 in all)" % (bad_row, rows.n) in str(e.value)
        # ---- a batch of four with proof 2 bad, and again under stream jitter (the GPU; the emulator has one stream and ignores it)
        for jitter, reps in ((0, 1), (300, 3)) if backend == "gpu" else ((0, 1),):
            ctx.tune("stream_jitter", jitter)
            for rep in range(reps):
                with pytest.raises(native.ZkhipError) as e:
                    prove_batch(ctx, scheme, pk, cs, zs, RNDS)
                assert e.value.code == -5, (jitter, rep)
                assert e.value.unsatisfied == ctx.unsatisfied() == [(2, bad_row, 1)], (jitter, rep)
                assert "proof 2 of 4: constraint %d of %d is not satisfied (1 in all)" % (bad_row, rows.n) in str(e.value)
                got = e.value.proofs
                assert [got[0], got[1], got[3]] == [plain[0], plain[1], plain[3]], (jitter, rep)
                assert got[2] == bytes(len(plain[2])), (jitter, rep)
                # the context stays usable: a good batch right behind it
                assert prove_batch(ctx, scheme, pk, cs, [zs[0]] * 4, RNDS) == plain, (jitter, rep)
                assert ctx.unsatisfied() == []
            ctx.tune("stream_jitter", 0)
        # two bad proofs of a batch, one of them with two failing rows: in proof order
        zb2, z2 = rows.assignment([cols[1][0], cols[rows.n - 1][2]])
        assert failing_rows(rows, z2) == [1, rows.n - 1]
        with pytest.raises(native.ZkhipError) as e:
            prove_batch(ctx, scheme, pk, cs, [zs[2], zs[0], native.Assignment(ctx, cs, zb2), zs[0]], RNDS)
        assert e.value.unsatisfied == [(0, bad_row, 1), (2, 1, 2)]
        assert e.value.proofs[1] == plain[1] and e.value.proofs[3] == plain[3] and not any(e.value.proofs[0]) and not any(e.value.proofs[2])
        assert ctx.set_checked(False) is True
        assert prove(ctx, scheme, pk, cs, zb, RNDS[2]) == plain_bad
    pk.close()
    cs.close()


# ------------------------------------------------------------------ the command line
def cli_files(tmp_path, lib):
    """def main(private field a, field b) -> (field, field): return a * b, a * b + b — and a witness whose ~out_0 is wrong."""
    prog = ir.Prog(BN254, [ir.Parameter(1, True), ir.Parameter(2, False)], [
        ir.Constraint([(1, 1)], [(2, 1)], [(3, 1)]),
        ir.Constraint([(0, 1)], [(3, 1)], [(-1, 1)]),
        ir.Constraint([(0, 1)], [(2, 1), (3, 1)], [(-2, 1)]),
    ], return_count=2)
    a, b = 7, 9
    paths = {k: str(tmp_path / k) for k in ("out", "witness", "witness.bad", "proving.key", "proof.json")}
    open(paths["out"], "wb").write(ir.serialize_prog(prog))
    open(paths["witness"], "wb").write(ir.serialize_witness({0: 1, 1: a, 2: b, 3: a * b, -1: a * b, -2: a * b + b}))
    open(paths["witness.bad"], "wb").write(ir.serialize_witness({0: 1, 1: a, 2: b, 3: a * b, -1: a * b + 1, -2: a * b + b}))
    ctx = native.Context(0, lib)
    cs = native.Program(open(paths["out"], "rb").read(), lib).constraint_system(ctx)
    native.setup_g16(ctx, cs, synth.toxic_waste(0)).tofile(paths["proving.key"])
    ctx.close()
    return paths


def cli_checks(paths, commands, env):
    for cmd in commands:
        run = lambda witness, *more: subprocess.run(cmd + ["generate-proof", "-i", paths["out"], "-w", paths[witness], "-p", paths["proving.key"], "-j",
                                                           paths["proof.json"], "--entropy", "e"] + list(more), capture_output=True, text=True, cwd=ROOT, env=env)
        r = run("witness")
        assert r.returncode == 0 and "checked" not in r.stdout, r.stderr
        proof = open(paths["proof.json"]).read()
        r = run("witness", "--check")
        assert r.returncode == 0 and "checked: the witness satisfies all 3 constraints" in r.stdout, r.stderr
        assert open(paths["proof.json"]).read() == proof
        # the wrong value: proved all the same without --check, as before; refused with the constraint and its variables with it
        os.remove(paths["proof.json"])
        r = run("witness.bad")
        assert r.returncode == 0 and json.load(open(paths["proof.json"]))["inputs"][1] == "0x" + (64).to_bytes(32, "big").hex(), r.stderr
        os.remove(paths["proof.json"])
        r = run("witness.bad", "--check")
        assert r.returncode != 0 and not os.path.exists(paths["proof.json"])
        assert "constraint 1 of 3 is not satisfied (1 in all)" in r.stderr and "~out_0" in r.stderr, r.stderr


def test_cli_check_on_emulator(tmp_path):
    from emu_util import EMU_LIB, emu_library
    exe = os.path.join(HERE, "_emu", "zkhip-cli-emu")
    paths = cli_files(tmp_path, emu_library())
    cli_checks(paths, ([exe], [os.sys.executable, "-m", "zokrates_amd.cli"]), dict(os.environ, ZKHIP_LIBRARY=EMU_LIB))
    # --verify after a --check that passed, against the key of another program: the one alternative left
    other = ir.Prog(BN254, [ir.Parameter(1, True), ir.Parameter(2, False)], [
        ir.Constraint([(1, 1)], [(2, 2)], [(3, 1)]),
        ir.Constraint([(0, 1)], [(3, 1)], [(-1, 1)]),
        ir.Constraint([(0, 1)], [(2, 1), (3, 1)], [(-2, 1)]),
    ], return_count=2)
    ctx = native.Context(0, emu_library())
    cs = native.Program(np.frombuffer(ir.serialize_prog(other), dtype=np.uint8), emu_library()).constraint_system(ctx)
    native.setup_g16(ctx, cs, synth.toxic_waste(0)).tofile(paths["proving.key"] + ".other")
    ctx.close()
    common = [exe, "generate-proof", "-i", paths["out"], "-w", paths["witness"], "-p", paths["proving.key"] + ".other", "-j", paths["proof.json"], "--verify"]
    r = subprocess.run(common, capture_output=True, text=True)
    assert r.returncode == 1 and "witness not satisfying the program, or a key for another program" in r.stderr
    r = subprocess.run(common + ["--check"], capture_output=True, text=True)
    assert r.returncode == 1 and "a key for another program" in r.stderr and "witness not satisfying" not in r.stderr


@GPU
def test_cli_check_on_gpu(tmp_path):
    exe = os.path.join(ROOT, "zokrates_amd", "zkhip-cli")
    cli_checks(cli_files(tmp_path, native.default_library()), ([exe],), dict(os.environ))
