"""Witnesses computed on the device: `zkhip_xplan_create`, `zkhip_xplan_dims`, `zkhip_compute_witness` (`k_exec_program`,
`k_exec_gather`, `k_exec_witness_file`) and the layers above them.

The reference of every assertion is `tests/exec_ref.py` — a big-integer restatement of `Interpreter::execute` / `execute_solver` over
`serde_model`'s statement values, which never calls the library — and `oracle/ir.py` (`ark_order`, `serialize_witness`,
`public_inputs_values`).  Programs are written with `serde_model.program_file`, systems are built from `ir.ark_order`.  No
tolerances: bytes, verdicts and error codes are compared for equality.

What a resident assignment holds is observed as tests/test_witness_device.py observes it: through `zkhip_r1cs_check` over a system
with one row per variable (z_v * ONE = expected * ONE), so a wrong element is named by its row.

Every case that touches a device runs on the emulator (`-m "not gpu"`: bn128 and bls12_381) and on the GPU (`-m gpu`: bls12_377 as
well)."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import exec_ref as X
import serde_model
from oracle import ir
from oracle.fields import BN254, BLS12_381, BLS12_377
from zokrates_amd import native, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NONE = (None, 0)
GPU = pytest.mark.gpu
BAD_ARG, PARSE, UNSATISFIED = -1, -2, -5
CURVE = {0: BN254, 1: BLS12_381, 2: BLS12_377}


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


# ------------------------------------------------------------------ programs and systems
def to_bytes(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8)


def csr(rows, m):
    rp, col, val = [0], [], []
    for row in rows:
        for c in sorted(row):
            assert 0 <= c < m
            col.append(c)
            val.append(row[c])
        rp.append(len(col))
    return (np.asarray(rp, dtype=np.uint64), np.asarray(col, dtype=np.uint32), to_bytes(val) if val else np.zeros(0, dtype=np.uint8))


def specials(r):
    return [0, 1, 2, r - 1, (1 << 64) - 1, 1 << 64, (r - 1) // 2]


class Built:
    """A program (parameters [(id, private)], serde_model statements) as `out` bytes, its system from the oracle's column order on
    a context, and — unless the test wants the refusal — its execution plan."""

    def __init__(self, ctx, curve_id, params, statements, return_count=0, plan=True):
        self.ctx, self.curve_id, self.curve = ctx, curve_id, CURVE[curve_id]
        self.r = self.curve.r
        self.arguments = [X.parameter(v, p) for v, p in params]
        self.params = list(params)
        self.statements = list(statements)
        self.return_count = return_count
        self.data = np.frombuffer(serde_model.program_file(self.r, self.arguments, self.statements, return_count), dtype=np.uint8)
        self.irp = X.ir_prog(self.curve, self.arguments, self.statements, return_count)
        self.l, self.w, self.order, rows = ir.ark_order(self.irp)
        self.m = self.l + self.w
        self.n = sum(1 for s in self.statements if not isinstance(s, str) and s[0] == "Constraint")
        self.cs = native.ConstraintSystem(ctx, curve_id, self.n, self.l, self.w, [csr(mat, self.m) for mat in rows])
        self.program = native.Program(self.data, ctx.lib)
        assert (self.program.n, self.program.l, self.program.w) == (self.n, self.l, self.w)
        self.plan = self.program.exec_plan(ctx, self.cs, self.data) if plan else None
        # the column every parameter binding takes (public: instance, private: witness, in argument order)
        self.param_col, ni, nw = [], 1, 0
        for _, private in params:
            self.param_col.append(self.l + nw if private else ni)
            nw, ni = nw + private, ni + (not private)
        # rows of the R1CS by statement number
        self.row_of, k = {}, 0
        for i, s in enumerate(self.statements):
            if not isinstance(s, str) and s[0] == "Constraint":
                self.row_of[i] = k
                k += 1

    def refused(self):
        with pytest.raises(native.ZkhipError) as e:
            self.program.exec_plan(self.ctx, self.cs, self.data)
        return e.value.code, str(e.value)

    def reference(self, rows):
        """[(witness, None) | (None, failing statement)] per instance"""
        return [X.execute(self.r, self.arguments, self.statements, row) for row in rows]

    def z(self, witness, row):
        """the expected assignment: column j holds the value of its variable; a binding of a repeated parameter that a later one
        shadows keeps the argument it was given"""
        z = [1] + [witness[v] for v in self.order[1:]]
        last = {}
        for k, (v, _) in enumerate(self.params):
            last[v] = k
        for k, (v, _) in enumerate(self.params):
            if last[v] != k:
                z[self.param_col[k]] = row[k] % self.r
        return z

    def inputs(self, witness, row):
        z = self.z(witness, row)
        pub = [z[self.param_col[k]] for k, (_, private) in enumerate(self.params) if not private]
        return to_bytes(pub + [witness[-(k + 1)] for k in range(self.return_count)]).tobytes()

    def variable_system(self, z):
        """one row per column j >= 1: z_j * ONE = expected * ONE"""
        a = [{j: 1} for j in range(1, self.m)]
        b = [{0: 1} for _ in range(1, self.m)]
        c = [{0: z[j]} if z[j] else {} for j in range(1, self.m)]
        return native.ConstraintSystem(self.ctx, self.curve_id, self.m - 1, self.l, self.w, [csr(mat, self.m) for mat in (a, b, c)])

    def run(self, rows, **kw):
        kw.setdefault("want_files", True)
        kw.setdefault("want_inputs", True)
        return self.ctx.compute_witness(self.plan, rows, **kw)

    def assert_all_good(self, rows, check_z=True):
        """every instance against the reference: the file, the inputs, the resident assignment element by element.  Returns the batch's
        (files, inputs) for comparisons between runs."""
        ref = self.reference(rows)
        got = self.run(rows)
        assert got.code == 0 and got.status == [0] * len(rows) and got.first_statement == [None] * len(rows) and got.first_row == [None] * len(rows)
        for i, ((w, bad), row) in enumerate(zip(ref, rows)):
            assert bad is None
            assert got.files[i] == ir.serialize_witness(w), i
            assert got.inputs[i] == self.inputs(w, row), i
            if self.return_count == len([v for v in w if v < 0]) and len(set(v for v, _ in self.params)) == len(self.params):
                assert got.inputs[i] == to_bytes(ir.public_inputs_values(self.irp, w)).tobytes()
            if check_z:
                vs = self.variable_system(self.z(w, row))
                assert vs.check(got.assignments[i]) == NONE, i
                vs.close()
                assert self.cs.check(got.assignments[i]) == NONE, i
        got.close()
        return got.files, got.inputs

    def close(self):
        if self.plan:
            self.plan.close()
        self.program.close()
        self.cs.close()


def draw(rnd, r, k, count, fixed=()):
    """`count` rows of k arguments: the fixed rows first, then values from the specials and random ones"""
    sp = specials(r)
    rows = [list(f) for f in fixed]
    while len(rows) < count:
        rows.append([rnd.choice(sp) if rnd.random() < 0.6 else rnd.randrange(r) for _ in range(k)])
    return rows[:count]


# ------------------------------------------------------------------ 1. every solver, at its edges, with lanes that disagree
def solver_program(name, r, n=None):
    """(params, statements, fixed argument rows): one directive and the constraints that bind its outputs.  Variables: 1.. the
    arguments (private), 10.. the outputs, 50.. helpers."""
    C, D = X.constraint, X.directive
    one = [(0, 1)]
    big = [r - 1, (1 << 64) - 1, 1 << 64, (r - 1) // 2]
    if name == "ConditionEq":
        # x * inv = b;  (1 - b) * x = 0
        return [(1, True)], [D([([(1, 1)], one)], [10, 11], name), C([(1, 1)], [(11, 1)], [(10, 1)]), C([(0, 1), (10, r - 1)], [(1, 1)], [])], [[0], [1], [r - 1]]
    if name == "Div":
        # t = q * b;  (t - a) * b = 0
        return ([(1, True), (2, True)], [D([([(1, 1)], one), ([(2, 1)], one)], [10], name), C([(10, 1)], [(2, 1)], [(50, 1)]), C([(50, 1), (1, r - 1)], [(2, 1)], [])],
                [[5, 0], [0, 0], [7, 1], [1, r - 1]] + [[b, 0] for b in big])
    if name == "EuclideanDiv":
        # t = q * d;  (t + rem - n) * 1 = 0
        return ([(1, True), (2, True)], [D([([(1, 1)], one), ([(2, 1)], one)], [10, 11], name), C([(10, 1)], [(2, 1)], [(50, 1)]),
                                         C([(50, 1), (11, 1), (1, r - 1)], one, [])],
                [[5, 0], [0, 0], [r - 1, 0], [7, 1], [r - 1, 1], [3, 5], [1 << 64, r - 1], [r - 1, 1 << 64], [r - 1, 2], [(r - 1) // 2, (1 << 64) - 1], [6, 6], [r - 1, r - 1]])
    if name in ("Xor", "Or"):
        k = 2 if name == "Xor" else 1
        return ([(1, True), (2, False)], [D([([(1, 1)], one), ([(2, 1)], one)], [-1], name), C([(1, 1)], [(2, 1)], [(50, 1)]),
                                          C([(1, 1), (2, 1), (50, r - k)], one, [(-1, 1)])], [[0, 0], [0, 1], [1, 0], [1, 1]])
    if name == "ShaAndXorAndXorAnd":
        # bc = b * c;  (2 bc - b - c) * a = bc - o
        return ([(1, True), (2, True), (3, True)], [D([([(k, 1)], one) for k in (1, 2, 3)], [10], name), C([(2, 1)], [(3, 1)], [(50, 1)]),
                                                    C([(50, 2), (2, r - 1), (3, r - 1)], [(1, 1)], [(50, 1), (10, r - 1)])], [[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    if name == "ShaCh":
        return ([(1, True), (2, True), (3, True)], [D([([(k, 1)], one) for k in (1, 2, 3)], [10], name), C([(1, 1)], [(2, 1), (3, r - 1)], [(10, 1), (3, r - 1)])],
                [[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    assert name == "Bits"
    outs = [100 + i for i in range(n)]
    st = [D([([(1, 1)], one)], outs, ("Bits", n))] + [C([(o, 1)], [(o, 1)], [(o, 1)]) for o in outs]
    if n >= r.bit_length():
        st.append(C([(o, pow(2, n - 1 - i, r)) for i, o in enumerate(outs) if n - 1 - i < 256], one, [(1, 1)]))      # the bits make the integer up
    return [(1, True)], st, [[0], [1], [r - 1], [(1 << n) - 1 if (1 << n) - 1 < r else r - 2]]


SOLVERS = ["ConditionEq", "Div", "EuclideanDiv", "Xor", "Or", "ShaAndXorAndXorAnd", "ShaCh"]


@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("solver", SOLVERS)
def test_every_solver_at_its_edges(contexts, backend, curve_id, solver):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    params, statements, fixed = solver_program(solver, r)
    b = Built(ctx, curve_id, params, statements, return_count=1 if solver in ("Xor", "Or") else 0)
    assert b.plan.n_directives == 1 and b.plan.n_args == len(params) and b.plan.store_bytes == 32 * (b.m + b.plan.n_extra)
    rows = draw(random.Random(0xE0 + len(solver)), r, len(params), 65, fixed)
    b.assert_all_good(rows)
    b.close()


def bits_widths(r):
    return [1, 8, 32, 64, r.bit_length() - 1, r.bit_length(), 256, 300]


@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("which", range(8))
def test_bits_at_every_width(contexts, backend, curve_id, which):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    n = bits_widths(r)[which]
    params, statements, fixed = solver_program("Bits", r, n)
    b = Built(ctx, curve_id, params, statements)
    assert b.plan.n_directives == 1 and b.plan.n_checks == n + (n >= r.bit_length())
    rows = draw(random.Random(0xB0 + n), r, 1, 65, fixed)
    # the first output is the most significant bit kept
    w, _ = b.reference([[r - 1]])[0]
    assert w[100] == ((r - 1) >> (n - 1)) & 1 if n <= 256 else w[100] == 0
    b.assert_all_good(rows)
    b.close()


# ------------------------------------------------------------------ 2. define against check, on raw combinations
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_define_against_check(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    C, D = X.constraint, X.directive
    one = [(0, 1)]
    rnd = random.Random(0xDC)
    # a define, then the same term as a check; an empty left; duplicates that cancel; a zero coefficient
    st = [C([(1, 1)], [(2, 1)], [(3, 1)]),                          # 0: _2 = a * b            (define)
          C([(1, 1)], [(2, 1)], [(3, 1)]),                          # 1: a * b == _2           (check)
          C([], [(2, 1)], [(4, 1)]),                                # 2: _3 = 0 * b            (define, empty left)
          C([(4, 1)], one, []),                                     # 3: _3 * 1 == 0           (check, empty lin)
          C([(1, 1), (2, 5), (2, r - 5)], one, [(5, 1)]),           # 4: _4 = a + 5b - 5b      (define, duplicates that cancel)
          C([(5, 1)], one, [(1, 1), (3, 0)]),                       # 5: _4 == a + 0 * _2      (check, a zero coefficient)
          C([(1, 1), (9, 0)], one, [(9, 1)])]                       # 6: refused below: reads _8 (coefficient 0) before it is defined
    b = Built(ctx, curve_id, [(1, True), (2, False)], st[:6])
    assert (b.plan.n_defines, b.plan.n_checks, b.plan.n_statements, b.plan.n_extra) == (3, 3, 6, 0)
    b.assert_all_good(draw(rnd, r, 2, 5))
    b.close()
    code, msg = Built(ctx, curve_id, [(1, True), (2, False)], st, plan=False).refused()
    assert code == BAD_ARG and "statement 6" in msg and "_8" in msg
    # coefficient 2 on an undefined variable is a check, hence a read before definition; so are two terms of one undefined variable
    for lin, what in (([(3, 2)], "coefficient 2"), ([(3, 1), (3, 0)], "two terms"), ([(3, r - 1), (3, 2)], "two terms that sum to 1")):
        code, msg = Built(ctx, curve_id, [(1, True), (2, False)], [C([(1, 1)], [(2, 1)], lin)], plan=False).refused()
        assert code == BAD_ARG and "statement 0" in msg and "_2" in msg and "before" in msg, what
    # rows of 33 and of 600 terms (with repeats of a variable, kept raw)
    for terms in (33, 600):
        left = [(1 + (k % 3), rnd.randrange(r)) for k in range(terms)]
        b = Built(ctx, curve_id, [(1, True), (2, True), (3, False)], [C(left, [(2, 1), (0, 3)], [(7, 1)]), C(left, [(2, 1), (0, 3)], [(7, 1)]), C([(7, 1)], left, [(8, 1)])])
        assert (b.plan.n_defines, b.plan.n_checks) == (2, 1)
        b.assert_all_good(draw(rnd, r, 3, 3))
        b.close()
    # a directive output that overwrites an argument, and a later constraint that reads it; a variable with no column
    st = [D([([(1, 1)], [(2, 1)])], [1, 30], "ConditionEq"),        # _0 := (a b != 0), _29 := 1 / (a b): no constraint mentions _29
          C([(1, 1)], [(1, 1)], [(1, 1)]),                          # the new _0 is a bit (check: _0 is defined)
          D([([(30, 1)], one), ([(2, 1)], one)], [31], "Or"),       # reads _29, writes _30: neither has a column
          C([(1, 1)], [(2, 1)], [(-1, 1)])]                         # ~out_0 = _0 * b
    b = Built(ctx, curve_id, [(1, True), (2, False)], st, return_count=1)
    assert (b.plan.n_extra, b.plan.n_entries, b.plan.n_directives, b.m) == (2, 6, 2, 4)
    rows = draw(rnd, r, 2, 6, [[0, 5], [3, 0], [1, 1]])
    files, _ = b.assert_all_good(rows)
    w, _ = b.reference([rows[2]])[0]
    assert sorted(w) == [-1, 0, 1, 2, 30, 31] and w[1] == 1 and files[2] == ir.serialize_witness(w)
    b.close()
    # a repeated parameter keeps its last value; each binding has its own column
    for flags in ((True, False, True), (False, True, False), (True, True, True)):
        b = Built(ctx, curve_id, [(1, flags[0]), (2, flags[1]), (1, flags[2])], [C([(1, 1)], [(2, 1)], [(3, 1)]), C([(1, 1)], one, [(1, 1)])])
        assert b.plan.n_args == 3 and b.plan.n_entries == 4 and b.m == 5
        rows = [[7, 3, 9], [0, 1, r - 1], [r - 1, r - 1, 2]]
        b.assert_all_good(rows)
        w, _ = b.reference([rows[0]])[0]
        assert w[1] == 9 and w[3] == 27
        b.close()


# ------------------------------------------------------------------ 3. random straight-line programs
def random_program(r, seed, statements):
    """defines, checks that hold for every argument, directives of every supported solver, and logs; three arguments, two outputs"""
    rnd = random.Random(seed)
    C, D = X.constraint, X.directive
    defined = [0, 1, 2, 3]
    fresh = [10]

    def new():
        fresh[0] += 1
        return fresh[0]

    def comb(k=None):
        k = rnd.choice([0, 1, 1, 2, 2, 3, 5]) if k is None else k
        return [(rnd.choice(defined), rnd.choice([1, 1, r - 1, 2, 0, rnd.randrange(r)])) for _ in range(k)]

    st = []
    while len(st) < statements - 2:
        what = rnd.random()
        if what < 0.45:
            left, right, v = comb(), comb(), new()
            st.append(C(left, right, [(v, 1)]))
            defined.append(v)
            if rnd.random() < 0.5:
                st.append(C(left, right, [(v, 1)] if rnd.random() < 0.5 else [(v, 2), (v, r - 1), (defined[1], 0)]))
        elif what < 0.5:
            st.append(X.log())
        else:
            name = rnd.choice(["ConditionEq", "Bits", "Div", "Xor", "Or", "ShaAndXorAndXorAnd", "ShaCh", "EuclideanDiv"])
            n_in, n_out = (1, rnd.choice([1, 3, 16, 70])) if name == "Bits" else X.SIGNATURES[name]
            outs = [new() for _ in range(n_out)]
            st.append(D([(comb(rnd.choice([1, 2])), comb(rnd.choice([1, 2]))) for _ in range(n_in)], outs, ("Bits", n_out) if name == "Bits" else name))
            defined.extend(outs)
    st.append(C(comb(2), comb(2), [(-2, 1)]))
    st.append(C([(-2, 1)], comb(2), [(-1, 1)]))
    return [(1, True), (2, False), (3, True)], st


@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("statements", [200, 2000])
def test_random_programs(contexts, backend, curve_id, statements):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    params, st = random_program(r, 0x5EED + statements + curve_id, statements)
    b = Built(ctx, curve_id, params, st, return_count=2)
    assert b.plan.n_directives > statements // 4 and b.plan.n_defines > statements // 5 and b.plan.n_checks > statements // 20 and b.plan.n_extra > 0
    rnd = random.Random(statements)
    rows = draw(rnd, r, 3, 130)
    ref = b.reference(rows)
    want_files = [ir.serialize_witness(w) for w, _ in ref]
    want_inputs = [b.inputs(w, row) for (w, _), row in zip(ref, rows)]
    assert len(set(want_files)) > 100
    for count in (1, 2, 63, 64, 65, 130):
        got = b.run(rows[:count])
        assert got.code == 0 and got.files == want_files[:count] and got.inputs == want_inputs[:count]
        for i in sorted({0, count - 1, 63 % count}):
            assert b.cs.check(got.assignments[i]) == NONE
            vs = b.variable_system(b.z(ref[i][0], rows[i]))
            assert vs.check(got.assignments[i]) == NONE
            vs.close()
        got.close()
    # the chunk seams: the same bytes as in one chunk
    try:
        for chunk, count in ((3, 7), (64, 130), (1, 3)):
            ctx.tune("exec_chunk", chunk)
            got = b.run(rows[:count])
            assert got.code == 0 and got.files == want_files[:count] and got.inputs == want_inputs[:count]
            for i in (0, count - 1):
                assert b.cs.check(got.assignments[i]) == NONE
            got.close()
    finally:
        ctx.tune("exec_chunk", 0)
    b.close()


# ------------------------------------------------------------------ 4. failing instances
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_failing_instances(contexts, backend, curve_id):
    """a program whose checks hold unless an argument says otherwise: _0 picks the failing checks (1: the first, 2: the second, 3: both)"""
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    C, D = X.constraint, X.directive
    one = [(0, 1)]
    st = [C([(2, 1)], [(3, 1)], [(10, 1)]),                                   # 0: define
          X.log(),                                                            # 1
          D([([(2, 1)], one), ([(3, 1)], one)], [11], "Xor"),                 # 2
          C([(1, 1)], [(1, 1), (0, r - 2)], []),                              # 3: a (a - 2) == 0: fails for a = 1, 3        (R1CS row 1)
          C([(10, 1)], one, [(12, 1)]),                                       # 4: define
          X.log(),                                                            # 5
          C([(1, 1)], [(1, 1), (0, r - 1)], []),                              # 6: a (a - 1) == 0: fails for a = 2, 3        (R1CS row 3)
          C([(12, 1)], [(11, 1)], [(-1, 1)])]                                 # 7: define the output
    b = Built(ctx, curve_id, [(1, False), (2, True), (3, True)], st, return_count=1)
    assert b.row_of == {0: 0, 3: 1, 4: 2, 6: 3, 7: 4}
    rnd = random.Random(0xFA)
    base = [[0] + draw(rnd, r, 2, 1)[0] for _ in range(130)]
    good_files, good_inputs = b.assert_all_good(base, check_z=False)
    zero_file = bytes(b.plan.file_bytes)
    try:
        for chunk in (0, 64):
            ctx.tune("exec_chunk", chunk)
            for bad in ({0: 1}, {129: 2}, {63: 1}, {64: 2}, {64: 3}, {0: 3, 63: 2, 64: 1, 65: 1, 127: 3, 128: 2}):
                rows = [list(row) for row in base]
                for k, a in bad.items():
                    rows[k][0] = a
                ref = b.reference(rows)
                got = b.run(rows)
                assert got.code == UNSATISFIED
                first = min(bad)
                want_st = {1: 3, 2: 6, 3: 3}
                for i in range(130):
                    if i in bad:
                        assert ref[i] == (None, want_st[bad[i]])
                        assert (got.status[i], got.first_statement[i], got.first_row[i]) == (UNSATISFIED, want_st[bad[i]], b.row_of[want_st[bad[i]]])
                        assert got.assignments[i] is None and got.files[i] == zero_file and got.inputs[i] == bytes(64)
                    else:
                        assert (got.status[i], got.first_statement[i], got.first_row[i]) == (0, None, None)
                        assert got.files[i] == good_files[i] and got.inputs[i] == good_inputs[i] and b.cs.check(got.assignments[i]) == NONE
                s0 = want_st[bad[first]]
                assert got.message.startswith("instance %d does not satisfy the program: statement %d, constraint (R1CS row) %d; %d of 130" % (first, s0, b.row_of[s0], len(bad)))
                # zkhip_r1cs_check names the same row for the assignment the interpreter would have reached had it carried on
                w, _ = X.execute(r, b.arguments, [X.log() if k in (3, 6) else s for k, s in enumerate(st)], rows[first])
                assert b.cs.check(to_bytes(b.z(w, rows[first])))[0] == got.first_row[first]
                got.close()
    finally:
        ctx.tune("exec_chunk", 0)
    b.close()


# ------------------------------------------------------------------ 5. refusals
MoreSolvers = serde_model.Enum(ConditionEq=None, Bits=serde_model.USIZE, Zir=serde_model.Struct(("name", serde_model.STR)), Ref=serde_model.RefCall, Sha256Round=None,
                               SnarkVerifyBls12377=serde_model.USIZE, Poseidon=None)


def program_with_solver(r, solver_value, n_in=1, n_out=2):
    """`out` bytes of one directive with a solver serde_model's table does not know, encoded through a wider table of this file"""
    st = serde_model.Struct(("span", serde_model.Opt(serde_model.Span)), ("inputs", serde_model.Vec(serde_model.QuadComb)), ("outputs", serde_model.Vec(serde_model.Variable)),
                            ("solver", MoreSolvers))
    statement = serde_model.Enum(Constraint=serde_model.ConstraintStatement, Directive=st)
    directive = ("Directive", {"span": None, "inputs": [X.quad([(1, 1)], [(0, 1)]) for _ in range(n_in)], "outputs": [{"id": 10 + k} for k in range(n_out)], "solver": solver_value})
    keep = X.constraint([(1, 1)], [(1, 1)], [(2, 1)])
    # the file's framing as serde_model.program_file writes it (serialize.rs:202-279), around statements encoded through the wider table
    enc = serde_model.encode
    params = enc(serde_model.Vec(serde_model.Parameter), [X.parameter(1, True)])
    stmts = enc(statement, directive) + enc(statement, keep)
    solv = enc(serde_model.Vec(serde_model.Solver), [])
    modmap = bytes([0xa1]) + enc(serde_model.STR, "modules") + bytes([0xa0])
    off, secs = 120, b""
    for ty, blob in ((1, params), (2, stmts), (3, solv), (3, modmap)):
        secs += struct.pack("<IQQ", ty, off, len(blob))
        off += len(blob)
    header = b"ZOK\0" + bytes([3, 0, 0, 0]) + serde_model.field_id(r) + struct.pack("<II", 1, 0) + secs
    return np.frombuffer(header + b"\0" * (120 - len(header)) + params + stmts + solv + modmap, dtype=np.uint8)


@pytest.mark.parametrize("backend,curve_id", [on("emu", 0), on("emu", 1), on("gpu", 2)])
def test_refusals(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    C, D = X.constraint, X.directive
    one = [(0, 1)]
    keep = C([(1, 1)], [(1, 1)], [(2, 1)])
    base = Built(ctx, curve_id, [(1, True)], [keep])

    def plan_error(data):
        prog = native.Program(data, ctx.lib)
        with pytest.raises(native.ZkhipError) as e:
            prog.exec_plan(ctx, base.cs, data)
        prog.close()
        return e.value.code, str(e.value)

    # each unsupported solver by name
    for value, shown in ((("Zir", {"name": "f"}), "Zir"), (("Ref", {"index": 0, "signature": (1, 2)}), "Ref"), ("Sha256Round", "Sha256Round"),
                         (("SnarkVerifyBls12377", 1), "SnarkVerifyBls12377"), ("Poseidon", "Poseidon")):
        code, msg = plan_error(program_with_solver(r, value))
        assert code == BAD_ARG and "statement 0" in msg and ("solver " + shown + " keeps the host interpreter") in msg, msg
    good = program_with_solver(r, "ConditionEq")      # (the wider table writes a good program too)
    prog = native.Program(good, ctx.lib)
    plan = prog.exec_plan(ctx, base.cs, good)
    assert (plan.n_directives, plan.n_defines, plan.n_extra) == (1, 1, 2)
    plan.close()
    prog.close()
    # wrong input and output counts
    for inputs, outs, solver, says in ((2, 2, "ConditionEq", "takes 1 inputs and gives 2 outputs, the directive has 2 and 2"), (1, 1, "ConditionEq", "has 1 and 1"),
                                       (1, 7, ("Bits", 8), "gives 8 outputs"), (1, 1, "Div", "takes 2 inputs"), (2, 1, "EuclideanDiv", "gives 2 outputs"),
                                       (2, 1, "ShaCh", "takes 3 inputs")):
        st = [D([([(1, 1)], one)] * inputs, [10 + k for k in range(outs)], solver), keep]
        code, msg = Built(ctx, curve_id, [(1, True)], st, plan=False).refused()
        assert code == BAD_ARG and "statement 0" in msg and says in msg, msg
    # a read before definition: in a directive's input, in a constraint
    code, msg = Built(ctx, curve_id, [(1, True)], [keep, D([([(5, 1)], one)], [10, 11], "ConditionEq")], plan=False).refused()
    assert code == BAD_ARG and "statement 1 reads variable _4 before" in msg
    code, msg = Built(ctx, curve_id, [(1, True)], [C([(1, 1)], [(-3, 1)], [(2, 1)])], plan=False).refused()
    assert code == BAD_ARG and "statement 0 reads variable ~out_2 before" in msg
    # `out` bytes of another program than `prog`: another argument list, another constraint count, other variables, another curve, no program
    others = [Built(ctx, curve_id, [(1, False)], [keep], plan=False), Built(ctx, curve_id, [(1, True)], [keep, keep], plan=False),
              Built(ctx, curve_id, [(1, True)], [C([(1, 1)], [(1, 1)], [(3, 1)])], plan=False), Built(ctx, (curve_id + 1) % 3, [(1, True)], [keep], plan=False)]
    for other in others:
        with pytest.raises(native.ZkhipError) as e:
            base.program.exec_plan(ctx, base.cs, other.data)
        assert e.value.code == BAD_ARG and ("not the program the handle was parsed from" in str(e.value) or "another curve" in str(e.value)), str(e.value)
    with pytest.raises(native.ZkhipError) as e:
        base.program.exec_plan(ctx, others[1].cs, base.data)      # a system of another n
    assert e.value.code == BAD_ARG and "the constraint system has n = 2" in str(e.value)
    for cut in (50, 119, 130, base.data.size - 12, base.data.size - 40):      # (the solver list and the module map, 11 bytes at the end, are not read)
        with pytest.raises(native.ZkhipError) as e:
            base.program.exec_plan(ctx, base.cs, base.data[:cut])
        assert e.value.code in (PARSE, BAD_ARG)
    for other in others:
        other.close()
    L = ctx.lib.L
    import ctypes as CT
    h = CT.c_void_p()
    assert L.zkhip_xplan_create(ctx.h, base.program.h, base.cs.h, None, 0, CT.byref(h)) == BAD_ARG and "null argument" in L.zkhip_last_error(ctx.h).decode()
    assert L.zkhip_xplan_create(ctx.h, None, base.cs.h, native._ptr(base.data), base.data.size, CT.byref(h)) == BAD_ARG
    assert L.zkhip_xplan_create(None, base.program.h, base.cs.h, native._ptr(base.data), base.data.size, CT.byref(h)) == BAD_ARG
    assert L.zkhip_xplan_dims(None, None) == BAD_ARG and L.zkhip_xplan_dims(base.plan.h, None) == BAD_ARG
    # the call: an argument equal to r, caps too small, NULLs, a plan of another context, count == 0
    args = to_bytes([5, r, 7])
    status = np.zeros(3, dtype=np.int32)
    rc = L.zkhip_compute_witness(ctx.h, base.plan.h, 3, native._ptr(args), None, None, 0, None, 0, native._ptr(status), None, None)
    assert rc == PARSE and "instance 1, argument 0" in L.zkhip_last_error(ctx.h).decode()
    good = to_bytes([5, 6, 7])
    buf = np.zeros(3 * base.plan.file_bytes, dtype=np.uint8)
    rc = L.zkhip_compute_witness(ctx.h, base.plan.h, 3, native._ptr(good), None, native._ptr(buf), base.plan.file_bytes - 1, None, 0, native._ptr(status), None, None)
    assert rc == BAD_ARG and "witness buffer too small" in L.zkhip_last_error(ctx.h).decode() and not buf.any()
    pub = Built(ctx, curve_id, [(1, False)], [keep])
    rc = L.zkhip_compute_witness(ctx.h, pub.plan.h, 3, native._ptr(good), None, None, 0, native._ptr(buf), 0, native._ptr(status), None, None)
    assert rc == BAD_ARG and "inputs buffer too small" in L.zkhip_last_error(ctx.h).decode()
    pub.close()
    assert L.zkhip_compute_witness(ctx.h, base.plan.h, 3, native._ptr(good), None, None, 0, None, 0, None, None, None) == BAD_ARG
    assert L.zkhip_compute_witness(ctx.h, base.plan.h, 3, None, None, None, 0, None, 0, native._ptr(status), None, None) == BAD_ARG
    assert L.zkhip_compute_witness(ctx.h, None, 3, native._ptr(good), None, None, 0, None, 0, native._ptr(status), None, None) == BAD_ARG
    assert L.zkhip_compute_witness(None, base.plan.h, 3, native._ptr(good), None, None, 0, None, 0, native._ptr(status), None, None) == BAD_ARG
    assert L.zkhip_compute_witness(ctx.h, base.plan.h, 0, None, None, None, 0, None, 0, None, None, None) == 0
    # everything may be NULL but the status: the verdicts alone
    assert L.zkhip_compute_witness(ctx.h, base.plan.h, 3, native._ptr(good), None, None, 0, None, 0, native._ptr(status), None, None) == 0 and not status.any()
    second = native.Context(0, ctx.lib)
    rc = L.zkhip_compute_witness(second.h, base.plan.h, 3, native._ptr(good), None, None, 0, None, 0, native._ptr(status), None, None)
    assert rc == BAD_ARG and "another context" in L.zkhip_last_error(second.h).decode()
    second.close()
    for value in (-1, 65535 * 64 + 1):      # (above: more waves than the y of a grid holds)
        with pytest.raises(native.ZkhipError) as e:
            ctx.tune("exec_chunk", value)
        assert e.value.code == BAD_ARG
    ctx.tune("exec_chunk", 65535 * 64)
    ctx.tune("exec_chunk", 0)
    base.close()


def proving_program(r):
    """49 constraints over three public arguments, two private ones and two outputs: a domain of 2^6"""
    C, D = X.constraint, X.directive
    one = [(0, 1)]
    st = [D([([(4, 1)], one)], [20 + k for k in range(8)], ("Bits", 8))] + [C([(20 + k, 1)], [(20 + k, 1)], [(20 + k, 1)]) for k in range(8)]
    st += [D([([(1, 1)], one), ([(5, 1)], one)], [30], "Div"), C([(30, 1)], [(5, 1)], [(31, 1)]), D([([(2, 1), (3, 1)], one)], [32, 33], "ConditionEq"),
           C([(2, 1), (3, 1)], [(33, 1)], [(32, 1)])]
    prev = 31
    for k in range(36):
        st.append(C([(prev, 1), (20 + k % 8, 1)], [(1 + k % 5, 1), (0, k)], [(40 + k, 1)]))
        prev = 40 + k
    st += [C([(prev, 1)], [(32, 1)], [(-2, 1)]), C([(-2, 1)], [(30, 1)], [(-1, 1)])]
    return [(1, False), (4, True), (2, False), (5, True), (3, False)], st


@pytest.mark.parametrize("backend", BACKENDS)
def test_split_pending_refuses_and_open_queue_allows(contexts, backend):
    from oracle import cpu, groth16 as g16
    ctx = context(contexts, backend)
    r = BN254.r
    params, st = proving_program(r)
    b = Built(ctx, 0, params, st, return_count=2)
    assert b.n == 48 and b.plan.n_directives == 3
    rnd = random.Random(0x51)
    rows = [[rnd.randrange(r), rnd.randrange(256), rnd.randrange(r), 1 + rnd.randrange(r - 1), rnd.randrange(r)] for _ in range(5)]
    want_files, want_inputs = b.assert_all_good(rows)
    ref = b.reference(rows)
    pk = native.ProvingKey(ctx, 0, native.setup_g16(ctx, b.cs, synth.toxic_waste(0)))
    rr = [(0x1111 * (i + 1), 0x2222 * (i + 3)) for i in range(5)]
    want = [native.prove_g16(ctx, pk, b.cs, to_bytes(b.z(w, row)), *rnd_) for (w, _), row, rnd_ in zip(ref, rows, rr)]
    # while a queue is open: allowed, and the queue's proofs are unchanged
    with native.ProofQueue(ctx, pk, b.cs) as q:
        q.submit(to_bytes(b.z(ref[0][0], rows[0])), rr[0])
        got = b.run(rows)
        assert got.code == 0 and got.files == want_files and got.inputs == want_inputs
        q.submit(got.assignments[1], rr[1])
        again = b.run(rows[2:])
        q.submit(again.assignments[0], rr[2])
        proofs = [q.collect()[1] for _ in range(3)]
        assert proofs == want[:3]
        with pytest.raises(native.ZkhipError) as e:      # (the plan itself enqueues copies: made before the queue is opened)
            b.program.exec_plan(ctx, b.cs, b.data)
        assert e.value.code == BAD_ARG and "proof queue is open" in str(e.value)
        got.close()
        again.close()
    pk.close()
    # while a split proof is pending: refused, and the pending proof is as it was
    oc = cpu.Circuit.synth(0, 29, 0x5EED00F1)
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
    with pytest.raises(native.ZkhipError) as e:
        b.run(rows)
    assert e.value.code == BAD_ARG and "split proof is pending" in str(e.value)
    with pytest.raises(native.ZkhipError) as e:
        b.program.exec_plan(ctx, b.cs, b.data)
    assert e.value.code == BAD_ARG and "split proof is pending" in str(e.value)
    assert native.prove_g16_split_end(ctx, spk, cs, other).tobytes() == part.tobytes()
    assert b.run(rows).files == want_files
    spk.close()
    cs.close()
    b.close()


# ------------------------------------------------------------------ 6. the same proofs
PROOFS = [on("emu", "g16", 0), on("emu", "gm17", 1), on("gpu", "g16", 0), on("gpu", "g16", 1), on("gpu", "g16", 2), on("gpu", "gm17", 0), on("gpu", "gm17", 1),
          on("gpu", "gm17", 2)]


@pytest.mark.parametrize("backend,scheme,curve_id", PROOFS)
def test_same_proofs(contexts, backend, scheme, curve_id):
    """proofs from compute_witness handles through prove_*_resident, _resident_batch and ProofQueue.submit equal the proofs from the
    reference's z through prove_g16 / prove_gm17, byte for byte: key unbound and bound, checked mode on"""
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    params, st = proving_program(r)
    b = Built(ctx, curve_id, params, st, return_count=2)
    assert b.n <= 64
    tox = synth.toxic_waste(curve_id)
    raw = native.setup_gm17(ctx, b.cs, (tox[0], tox[1], tox[2], tox[4])) if scheme == "gm17" else native.setup_g16(ctx, b.cs, tox)
    pk = native.ProvingKey(ctx, curve_id, raw, scheme=scheme)
    rnd = random.Random(0x6A + curve_id)
    rows = [[rnd.randrange(r), rnd.randrange(256), rnd.randrange(r), 1 + rnd.randrange(r - 1), rnd.randrange(r)] for _ in range(4)]
    rr = [(0x1111 * (i + 1), 7 + i, 0x2222 * (i + 3)) if scheme == "gm17" else (0x1111 * (i + 1), 0x2222 * (i + 3)) for i in range(4)]
    zs = [to_bytes(b.z(w, row)) for (w, _), row in zip(b.reference(rows), rows)]
    host = native.prove_gm17 if scheme == "gm17" else native.prove_g16

    def resident(a, rnd_):
        return native.prove_gm17(ctx, pk, b.cs, a, *rnd_) if scheme == "gm17" else native.prove_g16_resident(ctx, pk, b.cs, a, *rnd_)

    assert ctx.set_checked(None) is False
    try:
        for bound, checked in ((False, False), (True, False), (True, True)):
            if bound and not pk.is_bound(b.cs):
                pk.bind(b.cs)
            ctx.set_checked(checked)
            want = [host(ctx, pk, b.cs, z, *x) for z, x in zip(zs, rr)]
            assert len(set(want)) == 4
            got = b.run(rows, want_files=False, want_inputs=False)
            assert [resident(a, x) for a, x in zip(got.assignments, rr)] == want
            batch = native.prove_gm17_resident_batch if scheme == "gm17" else native.prove_g16_resident_batch
            assert batch(ctx, pk, b.cs, got.assignments, rr)[0] == want
            with native.ProofQueue(ctx, pk, b.cs) as q:
                for a, x in zip(got.assignments[:3], rr):
                    q.submit(a, x)
                assert [q.collect()[1] for _ in range(3)] == want[:3]
            got.close()
    finally:
        ctx.set_checked(False)
    pk.close()
    b.close()


# ------------------------------------------------------------------ 7. the host layer and the CLI
def cli_checks(tmp_path, lib, exe, env):
    """`compute-witness` writes the reference's file and prints the return values; `generate-proof --arguments` writes the proof.json
    of `generate-proof -w` over that file; a failing check and an unsupported solver are errors, not files"""
    ctx = native.Context(0, lib)
    r = BN254.r
    params, st = proving_program(r)
    b = Built(ctx, 0, params, st, return_count=2, plan=False)
    paths = {k: str(tmp_path / k) for k in ("out", "proving.key", "witness", "proof.json", "proof2.json", "bad.out", "zir.out")}
    open(paths["out"], "wb").write(b.data.tobytes())
    native.setup_g16(ctx, b.cs, synth.toxic_waste(0)).tofile(paths["proving.key"])
    row = [12345678901234567890123, 201, r - 1, 77, 1 << 64]
    w, bad = b.reference([row])[0]
    assert bad is None
    args = [str(v) for v in row]
    run = lambda *a: subprocess.run([exe] + list(a), capture_output=True, text=True, cwd=ROOT, env=env)
    out = run("compute-witness", "-i", paths["out"], "-o", paths["witness"], "--verbose", "-a", *args)
    assert out.returncode == 0, out.stderr
    assert open(paths["witness"], "rb").read() == ir.serialize_witness(w)
    assert out.stdout == "Computing witness...\n\nWitness: \n[\"%d\",\"%d\"]\n\nWitness file written to '%s'\n" % (w[-1], w[-2], paths["witness"])
    for scheme in ("g16",):
        one = run("generate-proof", "-i", paths["out"], "-w", paths["witness"], "-p", paths["proving.key"], "-j", paths["proof.json"], "--entropy", "e", "-s", scheme)
        two = run("generate-proof", "-i", paths["out"], "-p", paths["proving.key"], "-j", paths["proof2.json"], "--entropy", "e", "-s", scheme, "--arguments", *args)
        assert one.returncode == 0 and two.returncode == 0 and "witness computed on the device from 5 arguments" in two.stdout, one.stderr + two.stderr
        assert open(paths["proof.json"], "rb").read() == open(paths["proof2.json"], "rb").read()
        os.remove(paths["proof2.json"])
    # an argument list of the wrong length, a value that is no number, a value at r
    assert run("compute-witness", "-i", paths["out"], "-o", paths["witness"], "-a", "1", "2").returncode == 1
    out = run("compute-witness", "-i", paths["out"], "-o", paths["witness"], "-a", "1", "2", "x", "4", "5")
    assert out.returncode == 1 and "Could not parse argument: x" in out.stderr
    out = run("compute-witness", "-i", paths["out"], "-o", paths["witness"], "-a", str(r), "2", "3", "4", "5")
    assert out.returncode == 1 and "instance 0, argument 0" in out.stderr
    # a program whose check fails for these arguments; a program with a solver the device does not run
    C = X.constraint
    failing = serde_model.program_file(r, [X.parameter(1, True)], [C([(1, 1)], [(1, 1)], [(2, 1)]), C([(2, 1)], [(0, 1)], [(0, 9)])], 0)
    open(paths["bad.out"], "wb").write(failing)
    os.remove(paths["witness"])
    out = run("compute-witness", "-i", paths["bad.out"], "-o", paths["witness"], "-a", "4")
    assert out.returncode == 1 and "Execution failed: statement 1 of the program (constraint 1) is not satisfied" in out.stderr and not os.path.exists(paths["witness"])
    assert run("compute-witness", "-i", paths["bad.out"], "-o", paths["witness"], "-a", "3").returncode == 0
    open(paths["zir.out"], "wb").write(program_with_solver(r, ("Zir", {"name": "f"})).tobytes())
    out = run("compute-witness", "-i", paths["zir.out"], "-o", paths["witness"], "-a", "3")
    assert out.returncode == 1 and "solver Zir keeps the host interpreter" in out.stderr
    b.close()
    ctx.close()


def test_cli_on_emulator(tmp_path):
    from emu_util import EMU_LIB, emu_library
    cli_checks(tmp_path, emu_library(), os.path.join(HERE, "_emu", "zkhip-cli-emu"), dict(os.environ, ZKHIP_LIBRARY=EMU_LIB))


@GPU
def test_cli_on_gpu(tmp_path):
    cli_checks(tmp_path, native.default_library(), os.path.join(ROOT, "zokrates_amd", "zkhip-cli"), os.environ)


# ------------------------------------------------------------------ 8. the host side of the plan, alone
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "asan-ubsan"])
def test_plan_compiler_stand_alone(tmp_path, flags):
    """tests/host/exec_plan.cpp: xplan.h compiled alone — well-formed programs against the counts this file states, then every
    truncation and a sweep of single-byte mutations of the statement sections (each must end in a plan or an IngestError)"""
    C, D = X.constraint, X.directive
    one = [(0, 1)]
    r = BN254.r
    st = [D([([(1, 1)], one)], [20 + k for k in range(8)], ("Bits", 8)), C([(20, 1)], [(20, 1)], [(20, 1)]), X.log(), C([(1, 1)], [(2, 1)], [(3, 1)]),
          C([(1, 1)], [(2, 1)], [(3, 1)]), D([([(3, 1)], one), ([(2, 1)], one)], [40, 41], "EuclideanDiv"), C([(40, 1), (1, 5), (1, r - 5)], [], [(-1, 1)])]
    params = [X.parameter(1, True), X.parameter(2, False)]
    path = tmp_path / "out"
    path.write_bytes(serde_model.program_file(r, params, st, 1))
    exe = str(tmp_path / "exec_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + list(flags) + ["-I", os.path.join(ROOT, "zokrates_amd", "csrc"), "-x", "c++",
                                                                                          os.path.join(HERE, "host", "exec_plan.cpp"), "-o", exe])
    l, w, order, _ = ir.ark_order(X.ir_prog(BN254, params, st, 1))
    # arguments, statements executed, defines, checks, directives, entries, variables without a column (_20 .. _26 and _40)
    out = subprocess.run([exe, str(path), "0", "4", "1", str(l), str(w), ",".join(str(v) for v in order), "2", "2", "6", "2", "2", "2", "15", "8"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 failures"), out.stdout + out.stderr
