"""Witness files on the device: `zkhip_wplan_create`, `zkhip_assignment_upload_witness` (`k_witness_claim`, `k_witness_gather`),
`zkhip_queue_submit_witness`, `zkhip_queue_collect_inputs` and the layers above them.

The reference of every assertion is `oracle/ir.py` (`serialize_prog`, `serialize_witness`, `ark_order`, `public_inputs_values`) and
plain integers — never the library's own reader, except where a test says that two routes of the library must give the same BYTES
(the proofs).  No tolerances: bytes, verdicts and error codes are compared for equality.

What a resident assignment holds is observed through `zkhip_r1cs_check` over a system with one row per variable — the row of
variable v is z_v * ONE = (the expected value) * ONE — so a wrong element is named by its row.  The system is built from the
oracle's `ark_order`, not from the library's parse of the program.

Every case that touches a device runs on the emulator (`-m "not gpu"`: bn128 and bls12_381) and on the GPU (`-m gpu`: bls12_377 as
well); malformed files go to the emulator only."""
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from oracle import ir
from oracle.fields import BN254, BLS12_381, BLS12_377
from zokrates_amd import native, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NONE = (None, 0)
GPU = pytest.mark.gpu
BAD_ARG, PARSE, UNSATISFIED = -1, -2, -5
CURVE = {0: BN254, 1: BLS12_381, 2: BLS12_377}
M_LIST = (1, 2, 3, 255, 256, 257, 1023, 1025, 4099)
NON_CANONICAL = "non-canonical field element in the witness"
ID_RANGE = "variable id out of range in the witness"


def on(backend, *values):
    return pytest.param(backend, *values, marks=[GPU] if backend == "gpu" else [], id="-".join([backend] + [str(v) for v in values]))


DEVICES = [on("emu", 0), on("emu", 1), on("gpu", 0), on("gpu", 1), on("gpu", 2)]
BACKENDS = [on("emu"), on("gpu")]
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


# ------------------------------------------------------------------ files and systems, from the oracle
def to_bytes(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8)


def witness_file(entries, count=None):
    """The bytes of a `witness` file with `entries` = [(id, value)] in THIS order (values below 2^256); `count`: what the header says."""
    out = struct.pack("<Q", len(entries) if count is None else count)
    for vid, v in entries:
        out += struct.pack("<q", vid) + int(v).to_bytes(32, "little")
    return np.frombuffer(out, dtype=np.uint8)


def name(vid):
    return "~one" if vid == 0 else f"_{vid - 1}" if vid > 0 else f"~out_{-vid - 1}"


def csr(rows, m):
    """[{col: coeff}] per row -> (rowptr, col, val) as native.ConstraintSystem takes them"""
    rp, col, val = [0], [], []
    for row in rows:
        for c in sorted(row):
            assert 0 <= c < m
            col.append(c)
            val.append(row[c])
        rp.append(len(col))
    return (np.asarray(rp, dtype=np.uint64), np.asarray(col, dtype=np.uint32), to_bytes(val) if val else np.zeros(0, dtype=np.uint8))


class Case:
    """A program with one constraint per variable v (other than ~one): v * ONE = values[v] * ONE, in the order `ids`; its system on a
    context, from the oracle's column order.  Row k is the row of ids[k]."""

    def __init__(self, ctx, curve_id, public, private, n_out, others, seed):
        self.curve_id, self.curve = curve_id, CURVE[curve_id]
        r = self.curve.r
        rnd = random.Random(seed)
        outs = [-(k + 1) for k in range(n_out)]
        self.ids = list(public) + list(private) + outs[::-1] + list(others)      # (outputs first seen out of index order)
        assert len(set(self.ids)) == len(self.ids) and 0 not in self.ids
        special = [0, 1, r - 1, 2, (1 << 64) - 1, 1 << 64]
        self.values = {0: 1}
        self.values.update({v: rnd.choice(special) if rnd.random() < 0.4 else rnd.randrange(r) for v in self.ids})
        args = [ir.Parameter(v, False) for v in public] + [ir.Parameter(v, True) for v in private]
        rnd.shuffle(args)
        stmts = [ir.Constraint([(v, 1)], [(0, 1)], [(0, self.values[v])]) for v in self.ids]
        self.prog = ir.Prog(self.curve, args, stmts, return_count=n_out)
        self.l, self.w, self.order, rows = ir.ark_order(self.prog)
        self.m = self.l + self.w
        assert self.m == len(self.ids) + 1 and self.order[0] == 0
        self.column = {v: j for j, v in enumerate(self.order)}
        self.row = {v: k for k, v in enumerate(self.ids)}
        self.ctx = ctx
        self.cs = native.ConstraintSystem(ctx, curve_id, len(stmts), self.l, self.w, [csr(mat, self.m) for mat in rows])
        self.program = native.Program(np.frombuffer(ir.serialize_prog(self.prog), dtype=np.uint8), ctx.lib)
        assert (self.program.l, self.program.w, self.program.return_count) == (self.l, self.w, n_out)
        self.plan = self.program.plan(ctx, self.cs)

    def z(self, values=None):
        values = self.values if values is None else values
        return to_bytes([1] + [values[v] for v in self.order[1:]])

    def inputs(self, values=None):
        values = self.values if values is None else values
        return to_bytes(ir.public_inputs_values(self.prog, {v: x for v, x in values.items() if v in self.column})).tobytes()

    def entries(self, values=None, with_one=True):
        values = self.values if values is None else values
        return [(v, values[v]) for v in sorted(values) if with_one or v != 0]

    def upload(self, wit):
        """(verdict of the resident assignment over this system, inputs bytes); ZkhipError as the library raises it"""
        a, inputs = self.ctx.upload_witness(self.plan, wit)
        alone = self.ctx.upload_witness(self.plan, wit, want_inputs=False)
        got = self.cs.check(a)
        assert got == self.cs.check(alone)
        a.close()
        alone.close()
        return got, inputs.tobytes()

    def refused(self, wit):
        with pytest.raises(native.ZkhipError) as e:
            self.ctx.upload_witness(self.plan, wit)
        return e.value.code, str(e.value)

    def close(self):
        self.plan.close()
        self.program.close()
        self.cs.close()


def split_ids(m, sparse=False):
    """public arguments, private arguments, outputs, further variables of a system of m columns"""
    k = m - 1
    n_pub, n_priv, n_out = (2, 2, 2) if k >= 8 else (1, 1, 1) if k >= 3 else (min(k, 1), 0, 0)
    rest = k - n_pub - n_priv - n_out
    step = 37 if sparse else 1      # (sparse: gaps wider than the table's neighbours, and one id far out)
    pos = [1 + step * i for i in range(n_pub + n_priv + rest)]
    if sparse and rest:
        pos[-1] = 900000
    return pos[:n_pub], pos[n_pub:n_pub + n_priv], n_out, pos[n_pub + n_priv:]


# ------------------------------------------------------------------ 1. shapes and file orders
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_shapes_and_file_orders(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    for m in M_LIST:
        for sparse in ((False, True) if m in (3, 257, 1025) else (False,)):
            case = Case(ctx, curve_id, *split_ids(m, sparse), seed=0xC0 + m)
            assert case.m == m
            asc = case.entries()
            assert witness_file(asc).tobytes() == ir.serialize_witness(case.values)      # ascending: what the reference writes
            extras = [(1000001, 7), (-(case.prog.return_count + 1), r - 1), (-(case.prog.return_count + 40), 3), (777777, 0)]
            shuffled = list(asc)
            random.Random(m).shuffle(shuffled)
            files = {
                "ascending, count = m": asc,
                "without ~one": case.entries(with_one=False),
                "reversed": asc[::-1],
                "shuffled": shuffled,
                "extras, count > m": sorted(asc + extras),
                "extras first": extras + shuffled,
                "~one says 5": [(v, 5 if v == 0 else x) for v, x in asc],
            }
            assert len(asc) == m and len(files["extras, count > m"]) > m
            for what, entries in files.items():
                assert case.upload(witness_file(entries)) == (NONE, case.inputs()), (m, sparse, what)
            # a wrong element is named by its row: the first, the last, the neighbours of the workgroups' edges
            for k in sorted({0, 1, 254, 255, 256, 1022, 1023, 1024, m - 3, m - 2} & set(range(m - 1))):
                v = case.ids[k]
                changed = dict(case.values)
                changed[v] = (case.values[v] + 1) % r
                got, inputs = case.upload(witness_file(case.entries(changed)[::-1]))
                assert got == (k, 1) and inputs == case.inputs(changed), (m, sparse, k)
            case.close()


# ------------------------------------------------------------------ 2. repeated ids: the last in file order wins
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_repeated_ids(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    case = Case(ctx, curve_id, *split_ids(600), seed=0xD0B)
    base = case.entries()
    pub, priv, out = case.ids[0], case.ids[3], -1
    for v in (pub, priv, out, case.ids[-1]):
        good = case.values[v]
        wrong = [(good + 1 + i) % r for i in range(3)]
        others = [e for e in base if e[0] != v]
        for what, entries in {
            "twice": others[:10] + [(v, wrong[0])] + others[10:] + [(v, good)],
            "twice, adjacent": others[:300] + [(v, wrong[0]), (v, good)] + others[300:],
            "three times": [(v, wrong[0])] + others[:100] + [(v, wrong[1])] + others[100:400] + [(v, good)] + others[400:],
            # entries 255 | 256 of the file: the last work-item of one workgroup, the first of the next
            "across a workgroup boundary": others[:255] + [(v, wrong[2]), (v, good)] + others[255:],
            "across, far apart": others[:200] + [(v, wrong[0])] + others[200:520] + [(v, good)] + others[520:],
        }.items():
            assert entries.index((v, good)) > max(i for i, e in enumerate(entries) if e[0] == v and e[1] != good)
            if what.startswith("across a"):
                assert entries[255] == (v, wrong[2]) and entries[256] == (v, good)
            assert case.upload(witness_file(entries)) == (NONE, case.inputs()), (v, what)
            # ... and with the roles swapped the other value is the one that lands: its row fails
            swapped = [(e[0], wrong[0]) if e == (v, good) else e for e in entries]
            changed = dict(case.values)
            changed[v] = wrong[0]
            assert case.upload(witness_file(swapped)) == ((case.row[v], 1), case.inputs(changed)), (v, what)
    case.close()


# ------------------------------------------------------------------ 3. values at the edge of the field
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_values_at_the_modulus(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    case = Case(ctx, curve_id, *split_ids(300), seed=0xED6E)
    used = [case.ids[0], case.ids[5], case.ids[-1], -1]
    unused = [(4444, None), (-(case.prog.return_count + 3), None)]
    for ok in (0, 1, r - 1):
        for v in used:
            changed = dict(case.values)
            changed[v] = ok
            want = NONE if ok == case.values[v] else (case.row[v], 1)
            assert case.upload(witness_file(case.entries(changed))) == (want, case.inputs(changed)), (ok, v)
        for v, _ in unused:
            assert case.upload(witness_file(case.entries() + [(v, ok)])) == (NONE, case.inputs()), (ok, v)
    for bad in (r, r + 1, (1 << 256) - 1):
        for v in used:      # in an entry the system uses (first, middle, last work-item's neighbourhood)
            entries = [(e[0], bad) if e[0] == v else e for e in case.entries()]
            assert case.refused(witness_file(entries)) == (PARSE, f"zkhip error {PARSE} (PARSE): {NON_CANONICAL}"), (bad, v)
        for v, _ in unused:      # ... and in one it does not
            for entries in (case.entries() + [(v, bad)], [(v, bad)] + case.entries()):
                code, msg = case.refused(witness_file(entries))
                assert code == PARSE and NON_CANONICAL in msg, (bad, v)
        # the context is usable afterwards
        assert case.upload(witness_file(case.entries())) == (NONE, case.inputs())
    case.close()


# ------------------------------------------------------------------ 4. what the device finds wrong with a file: one defect per file
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_missing_variables_and_id_range(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    case = Case(ctx, curve_id, *split_ids(520), seed=0x3155)
    base = case.entries()
    # missing variables, several at once: the message names the one of the LOWEST column, in the reader's spelling
    for gone in ([case.ids[7]], [case.ids[-1]], [-1], [-2, case.ids[300]], [case.ids[0]], [case.ids[300], case.ids[40], case.ids[519 - 1]],
                 [case.ids[2], -1, case.ids[100]], case.ids[250:270]):
        lowest = min(gone, key=lambda v: case.column[v])
        code, msg = case.refused(witness_file([e for e in base if e[0] not in gone]))
        assert code == UNSATISFIED and msg.endswith("assignment missing for variable " + name(lowest)), (gone, msg)
    # an empty file: every variable is missing, column 1 is the lowest
    code, msg = case.refused(witness_file([]))
    assert code == UNSATISFIED and msg.endswith("assignment missing for variable " + name(case.order[1]))
    # the range rule: an index (id, or -(id + 1)) at or above min(2^31, max(2^20, 64 count)) is refused, whether or not the system has
    # the variable; just below it the entry is one the system does not have, and is ignored
    count = len(base) + 1
    bound = max(1 << 20, 64 * count)
    assert bound == 1 << 20
    for inside in (bound - 1, -bound):
        assert case.upload(witness_file(base + [(inside, 1)])) == (NONE, case.inputs()), inside
    for outside in (bound, -bound - 1, 1 << 31, (1 << 63) - 1, -(1 << 63), -(1 << 40)):
        for entries in (base + [(outside, 1)], [(outside, 1)] + base):
            assert case.refused(witness_file(entries)) == (PARSE, f"zkhip error {PARSE} (PARSE): {ID_RANGE}"), outside
    # ... and where the count decides the bound: 16 500 entries, bound = 64 x 16 500
    pad = [(600000 + i, i) for i in range(16500 - len(base) - 1)]
    bound = 64 * 16500
    assert bound > 1 << 20
    for inside in (bound - 1, -bound):
        assert case.upload(witness_file(base + pad + [(inside, 1)])) == (NONE, case.inputs()), inside
    for outside in (bound, -bound - 1):
        assert case.refused(witness_file(base + pad + [(outside, 1)])) == (PARSE, f"zkhip error {PARSE} (PARSE): {ID_RANGE}"), outside
    # a PARSE condition wins over a missing variable
    r = CURVE[curve_id].r
    assert case.refused(witness_file(base[5:] + [(1 << 20, 1)]))[0] == PARSE
    assert case.refused(witness_file(base[5:] + [(123456, r)]))[0] == PARSE
    assert case.upload(witness_file(base)) == (NONE, case.inputs())
    case.close()


# ------------------------------------------------------------------ 5. what the host refuses before anything is enqueued (emulator only)
def test_framing_plan_refusals_and_foreign_plans():
    from emu_util import emu_library
    lib = emu_library()
    ctx = native.Context(0, lib)
    case = Case(ctx, 0, *split_ids(40), seed=0xF4A)
    good = witness_file(case.entries())
    pk = native.ProvingKey(ctx, 0, native.setup_g16(ctx, case.cs, synth.toxic_waste(0)))
    framing = {
        "empty": good[:0], "seven bytes": good[:7], "one byte short": good[:-1], "one entry short": good[:-40], "one byte long": np.concatenate([good, good[:1]]),
        "one entry long": np.concatenate([good, good[8:48]]), "count + 1": witness_file(case.entries(), count=case.m + 1),
        "count - 1": witness_file(case.entries(), count=case.m - 1), "count = 2^61": witness_file(case.entries(), count=1 << 61),
        "count = 2^64 - 1": witness_file(case.entries(), count=(1 << 64) - 1),
    }
    with native.ProofQueue(ctx, pk, case.cs) as q:
        for what, wit in framing.items():
            with pytest.raises(native.ZkhipError) as e:
                q.submit_witness(case.plan, wit, (1, 2))
            assert e.value.code == PARSE and "witness file" in str(e.value), what
            assert q.state() == (q.state()[0], 0), what      # no ticket consumed
        assert q.submit_witness(case.plan, good, (1, 2)) == 0
        q.collect()
    for what, wit in framing.items():
        code, msg = case.refused(wit)
        assert code == PARSE and "witness file" in msg, what
    assert case.upload(good) == (NONE, case.inputs())

    # programs the plan refuses: their callers keep the host reader
    def plan_error(prog, cs):
        p = native.Program(np.frombuffer(ir.serialize_prog(prog), dtype=np.uint8), lib)
        with pytest.raises(native.ZkhipError) as e:
            p.plan(ctx, cs if cs is not None else p.constraint_system(ctx))
        p.close()
        return e.value.code, str(e.value)

    one = lambda v: ir.Constraint([(v, 1)], [(0, 1)], [(0, 3)])
    repeated = ir.Prog(BN254, [ir.Parameter(1, True), ir.Parameter(2, False), ir.Parameter(1, True)], [one(1), one(2)], return_count=0)
    code, msg = plan_error(repeated, None)
    assert code == BAD_ARG and "consumed twice (repeated parameter)" in msg and "_0" in msg
    no_column = ir.Prog(BN254, [ir.Parameter(1, False)], [one(1), one(-1)], return_count=2)      # ~out_1 occurs in no constraint
    code, msg = plan_error(no_column, None)
    assert code == BAD_ARG and "~out_1" in msg and "no column" in msg
    other_l = Case(ctx, 0, [1, 2, 3, 4], [5], 1, list(range(6, 39)), seed=1)       # the same m, another l
    other_w = Case(ctx, 0, *split_ids(41), seed=2)
    other_curve = Case(ctx, 1, *split_ids(40), seed=3)
    assert other_l.m == case.m and other_l.l != case.l
    for other, word in ((other_l, "l = "), (other_w, "w = "), (other_curve, "curve")):
        code, msg = plan_error(case.prog, other.cs)
        assert code == BAD_ARG and word in msg, msg

    # a plan of another system is refused at submit, and consumes no ticket; a plan of another context at upload
    same_shape = Case(ctx, 0, *split_ids(40), seed=0xF4B)
    with native.ProofQueue(ctx, pk, case.cs) as q:
        for foreign in (same_shape, other_l, other_w):
            with pytest.raises(native.ZkhipError) as e:
                q.submit_witness(foreign.plan, good, (1, 2))
            assert e.value.code == BAD_ARG and "another constraint system" in str(e.value)
            assert q.state()[1] == 0
    ctx2 = native.Context(0, lib)
    elsewhere = Case(ctx2, 0, *split_ids(40), seed=0xF4A)
    with pytest.raises(native.ZkhipError) as e:
        ctx.upload_witness(elsewhere.plan, good)
    assert e.value.code == BAD_ARG and "another context" in str(e.value)
    # an inputs buffer that is too small
    a, n = native.C.c_void_p(), native.C.c_uint64()
    buf = np.zeros(32 * 8, dtype=np.uint8)
    rc = lib.L.zkhip_assignment_upload_witness(ctx.h, case.plan.h, native._ptr(good), good.size, native._ptr(buf), case.plan.n_inputs - 1, native.C.byref(n), native.C.byref(a))
    assert rc == BAD_ARG and not a.value and "inputs buffer too small" in lib.L.zkhip_last_error(ctx.h).decode()
    for c in (elsewhere, same_shape, other_l, other_w, other_curve, case):
        c.close()
    pk.close()
    ctx2.close()
    ctx.close()


# ------------------------------------------------------------------ 6. the same proofs
PROOFS = [on("emu", "g16", 0), on("emu", "g16", 1), on("emu", "gm17", 0), on("emu", "gm17", 1), on("gpu", "g16", 0), on("gpu", "g16", 1), on("gpu", "g16", 2),
          on("gpu", "gm17", 0), on("gpu", "gm17", 1), on("gpu", "gm17", 2)]


def proving_case(ctx, curve_id, scheme, seed=0x9A0F):
    """A domain of 2^6: 50 columns, three public arguments and two outputs (l = 6), 49 constraints"""
    case = Case(ctx, curve_id, [3, 9, 12], [1, 2], 2, [20 + 3 * i for i in range(42)], seed=seed)
    assert case.m == 50 and case.l == 6
    tox = synth.toxic_waste(curve_id)
    raw = native.setup_gm17(ctx, case.cs, (tox[0], tox[1], tox[2], tox[4])) if scheme == "gm17" else native.setup_g16(ctx, case.cs, tox)
    return case, native.ProvingKey(ctx, curve_id, raw, scheme=scheme)


def rnds(scheme, n):
    return [(0x1111 * (i + 1), 7 + i, 0x2222 * (i + 3)) if scheme == "gm17" else (0x1111 * (i + 1), 0x2222 * (i + 3)) for i in range(n)]


def prove(ctx, pk, cs, z, rnd):
    """One proof from a host assignment or a resident one, either scheme"""
    if pk.scheme == "gm17":
        return native.prove_gm17(ctx, pk, cs, z, *rnd)
    return native.prove_g16_resident(ctx, pk, cs, z, *rnd) if isinstance(z, native.Assignment) else native.prove_g16(ctx, pk, cs, z, *rnd)


def witnesses(case, n):
    """n witness files of the case's program (other values for its variables: they need not satisfy the system for the bytes to be
    compared), in changing file orders, with their assignments and inputs from the oracle"""
    r = case.curve.r
    out = []
    for i in range(n):
        rnd = random.Random(0xAB + i)
        values = {v: rnd.randrange(r) for v in case.values}
        values[0] = 1
        entries = case.entries(values)
        entries = [entries, entries[::-1], sorted(entries, key=lambda e: rnd.random())][i % 3] + [(-(3 + i), 5), (4000 + i, 1)]
        out.append((witness_file(entries), case.z(values), case.inputs(values)))
    return out


def reader_route(case, wit):
    """z and inputs as zkhip_prog_assignment gives them for a file without entries the system lacks (which the host reader counts
    among the outputs: the documented difference)"""
    return case.program.assignment(wit)


@pytest.mark.parametrize("backend,scheme,curve_id", PROOFS)
def test_same_proofs(contexts, backend, scheme, curve_id):
    """upload_witness + *_resident and a queue cycle over witness files give the bytes of the route through zkhip_prog_assignment, over
    an unbound and a bound key; inputs as the oracle's public_inputs_values."""
    ctx = context(contexts, backend)
    assert ctx.set_checked(None) is False
    case, pk = proving_case(ctx, curve_id, scheme)
    files = witnesses(case, 7)
    rr = rnds(scheme, 7)
    z0, in0 = reader_route(case, witness_file(case.entries()))
    assert z0.tobytes() == case.z().tobytes() and in0.tobytes() == case.inputs()
    for bound in (False, True):
        if bound:
            pk.bind(case.cs)
        assert pk.is_bound(case.cs) == bound
        want = [prove(ctx, pk, case.cs, z, rnd) for (_, z, _), rnd in zip(files, rr)]
        assert len(set(want)) == len(want)
        for (wit, z, inputs), rnd, proof in zip(files[:3], rr, want):
            a, got_inputs = ctx.upload_witness(case.plan, wit)
            assert got_inputs.tobytes() == inputs
            assert prove(ctx, pk, case.cs, a, rnd) == proof
            a.close()
        with native.ProofQueue(ctx, pk, case.cs) as q:      # submit x 3, collect, submit, collect ...
            got = []
            for k in range(3):
                assert q.submit_witness(case.plan, files[k][0], rr[k]) == k
            for k in range(3, 7):
                got.append(q.collect(want_inputs=True))
                assert q.submit_witness(case.plan, files[k][0], rr[k]) == k
            while q.state()[1]:
                got.append(q.collect(want_inputs=True))
            assert [g[0] for g in got] == list(range(7))
            assert [g[1] for g in got] == want
            assert [g[2].tobytes() for g in got] == [f[2] for f in files]
    pk.close()
    case.close()


@pytest.mark.parametrize("backend,scheme,curve_id", [p for p in PROOFS if p.values[2] != 1])
def test_queue_failures_and_mixed_sources(contexts, backend, scheme, curve_id):
    """A ticket that fails in the middle leaves its neighbours' bytes as they are, for each of the three defects; plain collect on a
    witness ticket; collect_inputs on tickets of other sources; witness, packed and plain submits in one queue."""
    ctx = context(contexts, backend)
    case, pk = proving_case(ctx, curve_id, scheme, seed=0x9A10)
    r = case.curve.r
    files = witnesses(case, 3)
    rr = rnds(scheme, 3)
    want = [prove(ctx, pk, case.cs, z, rnd) for (_, z, _), rnd in zip(files, rr)]
    base = case.entries()
    gone = case.order[4]
    defects = [
        (witness_file([e for e in base if e[0] not in (gone, case.order[30])]), UNSATISFIED, "assignment missing for variable " + name(gone)),
        (witness_file(base + [(9999, r)]), PARSE, NON_CANONICAL),
        (witness_file([(1 << 21, 0)] + base), PARSE, ID_RANGE),
    ]
    resident = native.Assignment(ctx, case.cs, files[2][1])
    with native.ProofQueue(ctx, pk, case.cs) as q:
        for bad, code, text in defects:
            q.submit_witness(case.plan, files[0][0], rr[0])
            t_bad = q.submit_witness(case.plan, bad, rr[1])
            q.submit_witness(case.plan, files[2][0], rr[2])
            first = q.collect(want_inputs=True)
            assert (first[1], first[2].tobytes()) == (want[0], files[0][2])
            with pytest.raises(native.ZkhipError) as e:
                q.collect(want_inputs=True)
            assert e.value.code == code and text in str(e.value) and e.value.ticket == t_bad
            third = q.collect()      # plain collect on a witness ticket: the proof, the inputs dropped
            assert third[1] == want[2]
            assert q.state()[1] == 0
        # the three kinds of source in one queue, in both orders around the witness ticket
        packed = native.pack_assignment(files[1][1], ctx.lib)
        q.submit_packed(packed, rr[1])
        q.submit_witness(case.plan, files[0][0], rr[0])
        q.submit(files[2][1], rr[2])
        a = q.collect(want_inputs=True)
        q.submit(resident, rr[2])
        b = q.collect(want_inputs=True)
        q.submit_witness(case.plan, files[1][0], rr[1])
        c, d, e = q.collect(want_inputs=True), q.collect(want_inputs=True), q.collect(want_inputs=True)
        assert [x[1] for x in (a, b, c, d, e)] == [want[1], want[0], want[2], want[2], want[1]]
        # (a ticket that was not submitted as a witness: no inputs — also in a slot a witness ticket used before)
        assert [x[2].tobytes() for x in (a, b, c, d, e)] == [b"", files[0][2], b"", b"", files[1][2]]
        resident.close()
    pk.close()
    case.close()


@pytest.mark.parametrize("backend,scheme,curve_id", [on("emu", "g16", 0), on("emu", "gm17", 1), on("gpu", "g16", 2), on("gpu", "gm17", 0)])
def test_checked_mode(contexts, backend, scheme, curve_id):
    """Checked mode works as for any other source: a witness that satisfies the system proves, one with a wrong value is refused and
    its row named, from the resident route and from the queue, and the neighbours' bytes stay."""
    ctx = context(contexts, backend)
    case, pk = proving_case(ctx, curve_id, scheme, seed=0x9A11)
    rr = rnds(scheme, 3)
    good = witness_file(case.entries()[::-1])
    v = case.ids[17]
    changed = dict(case.values)
    changed[v] = (case.values[v] + 1) % case.curve.r
    bad = witness_file(case.entries(changed))
    want = prove(ctx, pk, case.cs, case.z(), rr[0])
    assert ctx.set_checked(True) is False
    try:
        a, _ = ctx.upload_witness(case.plan, good)
        assert prove(ctx, pk, case.cs, a, rr[0]) == want
        a.close()
        a, _ = ctx.upload_witness(case.plan, bad)
        with pytest.raises(native.ZkhipError) as e:
            prove(ctx, pk, case.cs, a, rr[0])
        assert e.value.code == UNSATISFIED and e.value.unsatisfied == [(0, case.row[v], 1)]
        a.close()
        with native.ProofQueue(ctx, pk, case.cs) as q:
            q.submit_witness(case.plan, good, rr[0])
            t = q.submit_witness(case.plan, bad, rr[1])
            q.submit_witness(case.plan, good, rr[0])
            assert q.collect(want_inputs=True)[1] == want
            with pytest.raises(native.ZkhipError) as e:
                q.collect(want_inputs=True)
            assert e.value.code == UNSATISFIED and e.value.ticket == t and f"constraint {case.row[v]} of" in str(e.value)
            assert e.value.unsatisfied == [(0, case.row[v], 1)]
            got = q.collect(want_inputs=True)
            assert got[1] == want and got[2].tobytes() == case.inputs()
    finally:
        ctx.set_checked(False)
    pk.close()
    case.close()


# ------------------------------------------------------------------ 7. calls out of order
@pytest.mark.parametrize("backend", BACKENDS)
def test_calls_out_of_order(contexts, backend):
    from oracle import cpu
    from oracle import groth16 as g16
    ctx = context(contexts, backend)
    case, pk = proving_case(ctx, 0, "g16", seed=0x9A12)
    wit = witness_file(case.entries())
    rr = rnds("g16", 2)
    want = prove(ctx, pk, case.cs, case.z(), rr[0])
    # under an open queue: the plan cannot be made, nothing can be uploaded; both name the queue, and its proofs are untouched
    with native.ProofQueue(ctx, pk, case.cs) as q:
        q.submit_witness(case.plan, wit, rr[0])
        for _ in range(2):
            with pytest.raises(native.ZkhipError) as e:
                case.program.plan(ctx, case.cs)
            assert e.value.code == BAD_ARG and "proof queue is open" in str(e.value)
            assert case.refused(wit) == (BAD_ARG, str(e.value))
        # collect_inputs on a ticket that is no witness ticket
        q.submit(case.z(), rr[0])
        first, second = q.collect(want_inputs=True), q.collect(want_inputs=True)
        assert (first[1], first[2].tobytes()) == (want, case.inputs()) and (second[1], second[2].tobytes()) == (want, b"")
        # an inputs buffer that is too small spends no ticket
        t = q.submit_witness(case.plan, wit, rr[0])
        out, n, ticket = np.zeros(q.proof_bytes, dtype=np.uint8), native.C.c_uint64(7), native.C.c_uint64()
        buf = np.zeros(32 * 8, dtype=np.uint8)
        rc = ctx.lib.L.zkhip_queue_collect_inputs(q.h, native.C.byref(ticket), native._ptr(out), native._ptr(buf), case.plan.n_inputs - 1, native.C.byref(n), None)
        assert rc == BAD_ARG and n.value == 0 and q.state()[1] == 1
        got = q.collect(want_inputs=True)
        assert got[0] == t and got[1] == want and got[2].tobytes() == case.inputs()
    # freeing a plan and making it again; a plan freed while nothing of it is in flight
    for _ in range(3):
        case.plan.close()
        case.plan = case.program.plan(ctx, case.cs)
        assert case.upload(wit) == (NONE, case.inputs())
    second = case.program.plan(ctx, case.cs)      # two plans of one program side by side
    a, _ = ctx.upload_witness(second, wit)
    second.close()
    assert case.cs.check(a) == NONE and prove(ctx, pk, case.cs, a, rr[0]) == want
    a.close()
    pk.close()
    # under a pending split proof (a world of one shard, as tests/test_compact_assignment.py sets it up)
    oc = cpu.Circuit.synth(0, 29, 0x5EED00F0)
    raw = cpu.ProvingKey.setup(oc, cpu.toxic_bytes(g16.Toxic.from_seed(BN254))).serialize()
    z = oc.assignment()
    cs = native.ConstraintSystem(ctx, 0, oc.n, oc.l, oc.w, [oc.csr(k) for k in range(3)])
    spk = native.ProvingKey(ctx, 0, raw, rank=0, world=1)
    spk.bind_shard(cs, raw)
    other = native.prove_g16_split_begin(ctx, spk, cs, z, 91, 92, 1)
    native.prove_g16_split_abort(ctx)
    native.prove_g16_split_begin(ctx, spk, cs, z, 91, 92, 0)
    part = native.prove_g16_split_end(ctx, spk, cs, other)
    native.prove_g16_split_begin(ctx, spk, cs, z, 91, 92, 0)
    for _ in range(2):
        with pytest.raises(native.ZkhipError) as e:
            case.program.plan(ctx, case.cs)
        assert e.value.code == BAD_ARG and "split proof is pending" in str(e.value)
        assert case.refused(wit) == (BAD_ARG, str(e.value))
    assert native.prove_g16_split_end(ctx, spk, cs, other).tobytes() == part.tobytes()
    assert case.upload(wit) == (NONE, case.inputs())
    spk.close()
    cs.close()
    case.close()


# ------------------------------------------------------------------ 8. under stream jitter: one raw buffer, one owner array, three proofs in flight
@GPU
@pytest.mark.parametrize("scheme,curve_id", [("g16", 0), ("gm17", 1), ("g16", 2)])
def test_gpu_stream_jitter(scheme, curve_id):
    """The queue keeps three witness proofs in flight over ONE buffer of file bytes and ONE owner array per context.  With a spin
    kernel of random length ahead of half the enqueues, an ordering that is not carried by the stream shows as a wrong proof or wrong
    inputs.  Different witnesses of different lengths and orders alternate, so a late reader would see another file's bytes."""
    ctx = native.Context(0)
    case, pk = proving_case(ctx, curve_id, scheme, seed=0x9A13)
    pk.bind(case.cs)
    files = witnesses(case, 6)
    rr = rnds(scheme, 6)
    want = [prove(ctx, pk, case.cs, z, rnd) for (_, z, _), rnd in zip(files, rr)]
    ctx.tune("stream_jitter", 300)      # process-wide: switched off again below
    try:
        for wit, z, inputs in files[:2]:
            a, got = ctx.upload_witness(case.plan, wit)
            assert got.tobytes() == inputs
            a.close()
        with native.ProofQueue(ctx, pk, case.cs) as q:
            order = [k % 6 for k in range(24)]
            got = []
            for n, k in enumerate(order):
                if n >= 3:
                    got.append(q.collect(want_inputs=True))
                q.submit_witness(case.plan, files[k][0], rr[k])
            while q.state()[1]:
                got.append(q.collect(want_inputs=True))
            assert [g[1] for g in got] == [want[k] for k in order]
            assert [g[2].tobytes() for g in got] == [files[k][2] for k in order]
    finally:
        ctx.tune("stream_jitter", 0)
    pk.close()
    case.close()
    ctx.close()


# ------------------------------------------------------------------ 9. the host layer
def test_plan_builder_under_sanitizers(tmp_path):
    """tests/host/witness_plan.cpp under ASan + UBSan, a stand-alone program: the plan's two tables and input places, every refusal
    of the builder, and the framing checks over heap blocks of exactly the files' sizes."""
    exe = str(tmp_path / "witness_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "zokrates_amd", "csrc"), "-x", "c++", os.path.join(HERE, "host", "witness_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0 failures", out.stdout + out.stderr


def host_files(tmp_path, lib):
    """The files the compiled host layer reads: a program with public arguments and outputs (the proving case's), its Groth16 key, three
    witness files in three file orders, and a program with a repeated parameter."""
    ctx = native.Context(0, lib)
    case, pk = proving_case(ctx, 0, "g16", seed=0x9A14)
    pk.close()
    paths = {k: str(tmp_path / k) for k in ("out", "proving.key", "w0", "w1", "w2", "repeated.out", "proof.json")}
    open(paths["out"], "wb").write(ir.serialize_prog(case.prog))
    native.setup_g16(ctx, case.cs, synth.toxic_waste(0)).tofile(paths["proving.key"])
    base = case.entries()
    for k, entries in enumerate((base, base[::-1] + [(4000, 3)], sorted(base, key=lambda e: (e[0] * 7919) % 101))):
        open(paths["w%d" % k], "wb").write(witness_file(entries).tobytes())
    one = lambda v: ir.Constraint([(v, 1)], [(0, 1)], [(0, 3)])
    repeated = ir.Prog(BN254, [ir.Parameter(1, True), ir.Parameter(2, False), ir.Parameter(1, True)], [one(1), one(2)], return_count=0)
    open(paths["repeated.out"], "wb").write(ir.serialize_prog(repeated))
    case.close()
    ctx.close()
    return paths


def host_program_checks(tmp_path, lib, libdir, libname):
    exe = tmp_path / "witness_queue"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", os.path.join(HERE, "host", "witness_queue.cpp"),
                           os.path.join(ROOT, "zokrates_amd", "csrc", "host", "backend.cpp"), "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-l" + libname,
                           "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined", "-o", str(exe)])
    p = host_files(tmp_path, lib)
    out = subprocess.run([str(exe), p["out"], p["proving.key"], p["w0"], p["w1"], p["w2"], p["repeated.out"]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "witness queue host checks OK" in out.stdout, out.stdout + out.stderr


def test_host_layer_on_emulator(tmp_path):
    """Hip::set_device_witness: Hip::prove and Hip::Queue from equal StdRng seeds with the setting on and off — the same proof.json
    text; compact wins; a refused program falls back (tests/host/witness_queue.cpp, linked against the emulator build)."""
    from emu_util import EMU_DIR, emu_library
    host_program_checks(tmp_path, emu_library(), EMU_DIR, "zkhip_emu")


@GPU
def test_gpu_host_layer(tmp_path):
    lib = native.default_library()
    host_program_checks(tmp_path, lib, os.path.dirname(lib.path), "zkhip")


def cli_checks(paths, exe, env):
    run = lambda wit, *more: subprocess.run([exe, "generate-proof", "-i", paths["out"], "-w", paths[wit], "-p", paths["proving.key"], "-j", paths["proof.json"],
                                             "--entropy", "e"] + list(more), capture_output=True, text=True, cwd=ROOT, env=env)
    for wit in ("w0", "w1"):
        r = run(wit)
        assert r.returncode == 0 and "device witness" not in r.stdout, r.stderr
        proof = open(paths["proof.json"], "rb").read()
        assert len(json.loads(proof)["inputs"]) == 5
        os.remove(paths["proof.json"])
        for more, says in (((), "read on the device"), (("--check",), "read on the device"), (("--compact-witness",), "off (--compact-witness wins)")):
            r = run(wit, "--device-witness", *more)
            assert r.returncode == 0 and "device witness: " + says in r.stdout, r.stderr + r.stdout
            assert open(paths["proof.json"], "rb").read() == proof
            os.remove(paths["proof.json"])
    # a program without a plan: the flag changes nothing, and the run says which reader it used
    r = subprocess.run([exe, "generate-proof", "-i", paths["repeated.out"], "-w", paths["w0"], "-p", paths["proving.key"], "-j", paths["proof.json"], "--device-witness"],
                       capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 1 and "consumed twice" in r.stderr and not os.path.exists(paths["proof.json"])


def test_cli_device_witness_on_emulator(tmp_path):
    from emu_util import EMU_LIB, emu_library
    cli_checks(host_files(tmp_path, emu_library()), os.path.join(HERE, "_emu", "zkhip-cli-emu"), dict(os.environ, ZKHIP_LIBRARY=EMU_LIB))


@GPU
def test_cli_device_witness_on_gpu(tmp_path):
    cli_checks(host_files(tmp_path, native.default_library()), os.path.join(ROOT, "zokrates_amd", "zkhip-cli"), dict(os.environ))
