"""A lone witness across the device: the level-scheduled route of `zkhip_compute_witness` (`ZKHIP_TUNE_EXEC_WIDE`: `k_exec_begin`,
`k_exec_level`, `k_exec_levels_run`), `zkhip_xplan_levels`, `zkhip_exec_last` and the layers above them.

Every result is held byte for byte to `tests/exec_ref.py` (the big-integer restatement of the interpreter) AND to the one-lane route
of the same plan: witness file, public inputs, status, `first_statement`, `first_row`, and the assignment through `zkhip_r1cs_check`.
No tolerances.  Every case asserts the route its data took (`exec_last()[0] == 2`), and the plan's levels and the call's launch count
against `schedule` / `launches` below — the level and segment rules of include/zkhip.h restated over the statements, which never
call the library.  The programs, systems and drawings are those of tests/test_device_exec.py (`Built`, `solver_program`, `draw`).

The emulator half is `-m "not gpu"` (bn128, bls12_381); the device half `-m gpu` (bls12_377 as well).  The emulator runs the
work-items of a level in ascending order of (opcode, offset), so a hazard case is written with the WRITER's opcode below the reader's:
a schedule that puts both in one level then gives other bytes, not only another level count (profiles/device_exec_wide_checks.txt)."""
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

import exec_ref as X
import serde_model
from oracle import ir
from oracle.fields import BN254
from test_device_exec import BAD_ARG, CURVE, NONE, UNSATISFIED, Built, draw, proving_program, random_program, solver_program, to_bytes
from zokrates_amd import native, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GPU = pytest.mark.gpu
WIDE_MIN_DEFAULT = 1024      # include/zkhip.h: ZKHIP_TUNE_EXEC_WIDE_MIN
RUN_BLOCK = 256              # csrc/wexec.cuh: WX_RUN_BLOCK, the workgroup of k_exec_levels_run
C, D = X.constraint, X.directive
ONE = [(0, 1)]


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


# ------------------------------------------------------------------ the rules, restated
def schedule(params, statements):
    """The level of every instruction (the arguments first, then the statements that execute), by the rules of include/zkhip.h: the
    smallest L >= 1 above the last write of every variable read and above the last write and every reader of every variable
    written.  A binding of a repeated parameter has a column of its own; the name reads the last."""
    W, R = {0: 0}, {0: 0}
    levels = []

    def place(reads, writes):
        L = 1 + max([W[s] for s in reads] + [max(W.get(s, 0), R.get(s, 0)) for s in writes] + [0])
        for s in reads:
            R[s] = max(R[s], L)
        for s in writes:
            W[s], R[s] = L, 0
        levels.append(L)

    name = {}
    for k, (v, _) in enumerate(params):
        name[v] = ("binding", k)
    for k in range(len(params)):
        place([], [("binding", k)])
    key = lambda v: name.get(v, v)
    ids = lambda comb: [key(var["id"]) for var, _ in comb["value"]]
    quad = lambda q: ids(q["left"]) + ids(q["right"])
    for s in statements:
        if isinstance(s, str) or s[0] == "Log":
            continue
        kind, body = s
        if kind == "Constraint":
            value = body["lin"]["value"]
            if len(value) == 1 and value[0][1] == 1 and key(value[0][0]["id"]) not in W:
                place(quad(body["quad"]), [key(value[0][0]["id"])])
            else:
                place(quad(body["quad"]) + ids(body["lin"]), [])
        else:
            place([v for q in body["inputs"] for v in quad(q)], [key(o["id"]) for o in body["outputs"]])
    return levels


def widths(levels):
    count = Counter(levels)
    return [count[L] for L in range(1, max(levels) + 1)]


def levels_figures(levels):
    w = widths(levels)
    assert all(w)      # (a level nobody sits at cannot be: every level has a binding constraint one below)
    return (len(w), max(w), len(levels), sum(1 for x in w if x < 64))


def launches(w, wide_min):
    """a level of wide_min instructions or more is a launch of its own, every maximal run of narrower ones is one"""
    n, in_run = 0, False
    for x in w:
        narrow = x < wide_min
        n += (not narrow) or (not in_run)
        in_run = narrow
    return n


class tuned:
    def __init__(self, ctx, **knobs):
        self.ctx, self.knobs = ctx, knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            self.ctx.tune(k, v)

    def __exit__(self, *a):
        for k in self.knobs:
            self.ctx.tune(k, 0)


def expected_last(b, count, wide_min=0, chunk=0):
    """what `exec_last()` must say after a level-scheduled call over `count` instances of b's program"""
    chunks = 1 if not chunk else -(-count // min(chunk, count))
    return (2, chunks, launches(widths(schedule(b.params, b.statements)), wide_min or WIDE_MIN_DEFAULT), wide_min or WIDE_MIN_DEFAULT)


def same(got, want):
    assert (got.code, got.status, got.first_statement, got.first_row, got.files, got.inputs) == (want.code, want.status, want.first_statement, want.first_row, want.files,
                                                                                                 want.inputs)
    assert [a is None for a in got.assignments] == [a is None for a in want.assignments]


def both_routes(ctx, b, rows, wide_min=0, chunk=0, satisfies=True):
    """the wide route against exec_ref (status, statement, row, file, inputs, every element of z) and against the one-lane route; the
    plan's levels and the call's launches against the restatement.  `satisfies`: the final assignment satisfies the program's R1CS
    (not so where a directive overwrites a variable a constraint defined).  Returns the wide route's batch (closed)."""
    lv = schedule(b.params, b.statements)
    assert b.plan.levels() == levels_figures(lv)
    want_last = expected_last(b, len(rows), wide_min, chunk)
    with tuned(ctx, exec_chunk=chunk):
        one = b.run(rows)
        assert ctx.exec_last() == (1, want_last[1], 1, WIDE_MIN_DEFAULT)
        with tuned(ctx, exec_wide=1, exec_wide_min=wide_min):
            wide = b.run(rows)
            assert ctx.exec_last() == want_last
    same(wide, one)
    zero_file, zero_inputs = bytes(b.plan.file_bytes), bytes(32 * b.plan.n_inputs)
    for i, ((w, bad), row) in enumerate(zip(b.reference(rows), rows)):
        if bad is not None:
            assert (wide.status[i], wide.first_statement[i], wide.first_row[i]) == (UNSATISFIED, bad, b.row_of[bad]), i
            assert wide.assignments[i] is None and wide.files[i] == zero_file and wide.inputs[i] == zero_inputs, i
            continue
        assert (wide.status[i], wide.first_statement[i], wide.first_row[i]) == (0, None, None), i
        assert wide.files[i] == ir.serialize_witness(w), i
        assert wide.inputs[i] == b.inputs(w, row), i
        vs = b.variable_system(b.z(w, row))
        assert vs.check(wide.assignments[i]) == NONE, i
        vs.close()
        if satisfies:
            assert b.cs.check(wide.assignments[i]) == NONE, i
    assert wide.code == (UNSATISFIED if any(bad is not None for _, bad in b.reference(rows)) else 0)
    one.close()
    wide.close()
    return wide


# ------------------------------------------------------------------ 1. the shapes of a schedule
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_chain(contexts, backend, curve_id):
    """130 dependent defines: depth 131 with the argument's level, width 1 — one launch, a barrier between every pair of levels"""
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    st = [C([(1, 1)], [(1, 1), (0, 3)], [(10, 1)])] + [C([(10 + k - 1, 1), (0, k)], [(1, 1)], [(10 + k, 1)]) for k in range(1, 130)]
    b = Built(ctx, curve_id, [(1, True)], st)
    assert b.plan.levels() == (131, 1, 131, 131)
    both_routes(ctx, b, draw(random.Random(0xC4), r, 1, 3, [[2]]))
    assert ctx.exec_last()[2] == 1
    both_routes(ctx, b, [[5]], wide_min=1)      # every level a launch of its own
    assert ctx.exec_last()[2] == 131
    b.close()


def one_level(width):
    """`width` independent defines under the arguments' level"""
    return [(1, True), (2, False)], [C([(1, 1), (0, k)], [(2, 1), (1, k + 1)], [(10 + k, 1)]) for k in range(width)]


@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("width", [1, 63, 64, 65, RUN_BLOCK - 1, RUN_BLOCK, RUN_BLOCK + 1])
def test_levels_inside_a_run_launch(contexts, backend, curve_id, width):
    """the stride loop of k_exec_levels_run and its tail"""
    ctx = context(contexts, backend)
    params, st = one_level(width)
    b = Built(ctx, curve_id, params, st)
    assert b.plan.levels() == (2, max(width, 2), width + 2, 1 + (width < 64))
    both_routes(ctx, b, draw(random.Random(width), CURVE[curve_id].r, 2, 3))
    assert ctx.exec_last()[2] == 1
    b.close()


@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("width", [1, 63, 64, 65, 255, 256, 257])
def test_levels_as_grid_launches(contexts, backend, curve_id, width):
    """wide_min = 2: the arguments' level (2 wide) and the defines' are launches of k_exec_level of their own"""
    ctx = context(contexts, backend)
    params, st = one_level(width)
    b = Built(ctx, curve_id, params, st)
    both_routes(ctx, b, draw(random.Random(width), CURVE[curve_id].r, 2, 3), wide_min=2)
    assert ctx.exec_last()[2] == 2      # (a level of one is a run launch of its own behind the arguments' level)
    b.close()


@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_seams(contexts, backend, curve_id):
    """consecutive levels of width wide_min - 1, wide_min, wide_min + 1, wide_min - 1 at wide_min = 8: a run, two levels of their own
    back to back, a run — FOUR launches by the segment rules (a wide level is a launch of its own, so two of them are two)"""
    ctx = context(contexts, backend)
    params = [(1 + k, k % 2 == 0) for k in range(7)]
    st = [C([(1 + k % 7, 1)], [(1 + (k + 1) % 7, 1), (0, k)], [(20 + k, 1)]) for k in range(8)]
    st += [C([(20 + k % 8, 1)], [(20 + (k + 3) % 8, 1), (0, 1)], [(40 + k, 1)]) for k in range(9)]
    st += [C([(40 + k, 1), (40 + k + 2, 1)], [(1, 1)], [(60 + k, 1)]) for k in range(7)]
    b = Built(ctx, curve_id, params, st)
    assert widths(schedule(params, st)) == [7, 8, 9, 7] and launches([7, 8, 9, 7], 8) == 4
    both_routes(ctx, b, draw(random.Random(0x5E), CURVE[curve_id].r, 7, 3), wide_min=8)
    assert ctx.exec_last()[2] == 4
    both_routes(ctx, b, draw(random.Random(0x5F), CURVE[curve_id].r, 7, 2), wide_min=9)      # run (7, 8), level (9), run (7)
    assert ctx.exec_last()[2] == 3
    b.close()


# ------------------------------------------------------------------ 2. hazards
@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("wide_min", [0, 1])
def test_write_after_read(contexts, backend, curve_id, wide_min):
    """x defined, y = x * x and q = x / 1 read it, a ConditionEq overwrites x, z = x * 1: y and q hold the old x, z the new.  (Div's
    opcode is above ConditionEq's: in one level the emulator would run the writer first.)"""
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    st = [C([(1, 1)], [(1, 1), (0, 5)], [(10, 1)]),                   # x = a (a + 5)
          C([(10, 1)], [(10, 1)], [(11, 1)]),                         # y = x x
          D([([(10, 1)], ONE), (ONE, ONE)], [14], "Div"),             # q = x / 1
          D([([(1, 1)], ONE)], [10, 12], "ConditionEq"),              # x := (a != 0)
          C([(10, 1)], ONE, [(13, 1)])]                               # z = x
    b = Built(ctx, curve_id, [(1, True)], st)
    assert schedule(b.params, st) == [1, 2, 3, 3, 4, 5]
    rows = [[3], [0], [r - 1]]
    w, _ = b.reference(rows)[0]
    assert (w[11], w[14], w[10], w[13]) == (24 * 24, 24, 1, 1)
    both_routes(ctx, b, rows, wide_min=wide_min, satisfies=False)
    b.close()


@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("wide_min", [0, 1])
def test_write_after_write(contexts, backend, curve_id, wide_min):
    """two directives onto one variable with no reader between them: the later one wins.  (The earlier has the higher opcode.)"""
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    st = [D([([(1, 1)], ONE), ([(2, 1)], ONE)], [20], "Div"),         # v = a / b
          D([([(2, 1)], ONE)], [20, 22], "ConditionEq"),              # v := (b != 0)
          C([(20, 1)], ONE, [(23, 1)])]                               # z = v
    b = Built(ctx, curve_id, [(1, True), (2, True)], st)
    assert schedule(b.params, st) == [1, 1, 2, 3, 4]
    rows = [[6, 3], [5, 0], [r - 1, 2]]
    w, _ = b.reference(rows)[0]
    assert (w[20], w[23]) == (1, 1)
    both_routes(ctx, b, rows, wide_min=wide_min)
    b.close()


@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_repeated_parameter_and_an_output_that_is_an_input(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    for flags in ((True, False, True), (False, True, False), (True, True, True)):
        b = Built(ctx, curve_id, [(1, flags[0]), (2, flags[1]), (1, flags[2])], [C([(1, 1)], [(2, 1)], [(3, 1)]), C([(1, 1)], ONE, [(1, 1)])])
        rows = [[7, 3, 9], [0, 1, r - 1], [r - 1, r - 1, 2]]
        assert b.reference(rows)[0][0][3] == 27
        for wide_min in (0, 1):
            both_routes(ctx, b, rows, wide_min=wide_min)
        b.close()
    # a directive whose output is one of its own inputs, read again behind it; variables without a column
    st = [D([([(1, 1)], [(2, 1)])], [1, 30], "ConditionEq"), C([(1, 1)], [(1, 1)], [(1, 1)]), D([([(30, 1)], ONE), ([(2, 1)], ONE)], [31], "Or"),
          C([(1, 1)], [(2, 1)], [(-1, 1)])]
    b = Built(ctx, curve_id, [(1, True), (2, False)], st, return_count=1)
    assert schedule(b.params, st) == [1, 1, 2, 3, 3, 3]
    for wide_min in (0, 1, 2):
        both_routes(ctx, b, draw(random.Random(0x0A), r, 2, 6, [[0, 5], [3, 0], [1, 1]]), wide_min=wide_min)
    b.close()


# ------------------------------------------------------------------ 3. checks
@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("wide_min", [0, 1])
def test_failing_checks(contexts, backend, curve_id, wide_min):
    """the lowest failing statement whatever level met it first: statement 2 sits at level 4, statements 3 and 4 at level 2"""
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    st = [C([(2, 1)], [(2, 1)], [(10, 1)]),                           # 0: t = b b                       level 2
          C([(10, 1)], [(10, 1)], [(11, 1)]),                         # 1: u = t t                       level 3
          C([(11, 1)], [(1, 1), (0, r - 1)], []),                     # 2: u (a - 1) == 0                level 4   (row 2)
          C([(1, 1)], [(1, 1), (0, r - 1)], []),                      # 3: a (a - 1) == 0                level 2   (row 3)
          X.log(),
          C([(1, 1)], [(1, 1), (0, r - 2)], [])]                      # 5: a (a - 2) == 0                level 2   (row 4)
    b = Built(ctx, curve_id, [(1, False), (2, True)], st)
    assert schedule(b.params, st) == [1, 1, 2, 3, 4, 2, 2]
    rows = [[1, 7], [2, 1], [3, 1], [3, 0], [0, 0], [2, 0]]
    want = [5, 2, 2, 3, None, 3]      # [3, 0]: two failing checks in one level; [2, 1] and [3, 1]: the higher statement fails in the lower level
    assert [bad for _, bad in b.reference(rows)] == want
    got = both_routes(ctx, b, rows, wide_min=wide_min)
    assert got.code == UNSATISFIED and got.first_statement == want and got.first_row == [None if s is None else b.row_of[s] for s in want]
    assert got.message.startswith("instance 0 does not satisfy the program: statement 5, constraint (R1CS row) 4; 5 of 6")
    # one failing instance between two that run through
    got = both_routes(ctx, b, [[0, 0], [3, 0], [0, 0]], wide_min=wide_min)
    assert got.status == [0, UNSATISFIED, 0] and got.first_statement == [None, 3, None] and got.assignments[1] is None and got.files[1] == bytes(b.plan.file_bytes)
    b.close()


# ------------------------------------------------------------------ 4. every solver, Bits at its widths
@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("solver", ["ConditionEq", "Div", "EuclideanDiv", "Xor", "Or", "ShaAndXorAndXorAnd", "ShaCh"])
def test_every_solver_at_its_edges(contexts, backend, curve_id, solver):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    params, statements, fixed = solver_program(solver, r)
    b = Built(ctx, curve_id, params, statements, return_count=1 if solver in ("Xor", "Or") else 0)
    rows = draw(random.Random(0xE0 + len(solver)), r, len(params), 65, fixed)
    both_routes(ctx, b, rows)
    both_routes(ctx, b, rows[:5], wide_min=1)
    b.close()


@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("which", range(4))
def test_bits(contexts, backend, curve_id, which):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    n = [1, 32, r.bit_length(), 300][which]
    params, statements, fixed = solver_program("Bits", r, n)
    b = Built(ctx, curve_id, params, statements)
    rows = draw(random.Random(0xB0 + n), r, 1, 65, fixed)
    both_routes(ctx, b, rows)                          # the n checks behind the directive: one level of n
    both_routes(ctx, b, rows[:4], wide_min=2)
    b.close()


# ------------------------------------------------------------------ 5. random programs
@pytest.mark.parametrize("backend,curve_id", DEVICES)
@pytest.mark.parametrize("statements", [200, 2000])
def test_random_programs(contexts, backend, curve_id, statements):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    params, st = random_program(r, 0x5EED + statements + curve_id, statements)
    b = Built(ctx, curve_id, params, st, return_count=2)
    lv = schedule(params, st)
    assert b.plan.levels() == levels_figures(lv) and len(widths(lv)) > 10
    rows = draw(random.Random(statements), r, 3, 65)
    ref = b.reference(rows)
    want_files = [ir.serialize_witness(w) for w, _ in ref]
    want_inputs = [b.inputs(w, row) for (w, _), row in zip(ref, rows)]
    with tuned(ctx, exec_chunk=64):
        one = b.run(rows)
    assert ctx.exec_last() == (1, 2, 1, WIDE_MIN_DEFAULT) and one.files == want_files and one.inputs == want_inputs
    for wide_min in (0, 4):
        for count, chunk in ((1, 0), (3, 0), (65, 64)):
            with tuned(ctx, exec_wide=1, exec_wide_min=wide_min, exec_chunk=chunk):
                got = b.run(rows[:count])
                assert ctx.exec_last() == expected_last(b, count, wide_min, chunk)
            assert got.code == 0 and got.files == want_files[:count] and got.inputs == want_inputs[:count]
            if count == 65:
                same(got, one)
            for i in sorted({0, count - 1, 63 % count}):
                assert b.cs.check(got.assignments[i]) == NONE
                vs = b.variable_system(b.z(ref[i][0], rows[i]))
                assert vs.check(got.assignments[i]) == NONE
                vs.close()
            got.close()
    one.close()
    b.close()


# ------------------------------------------------------------------ 6. the same proofs
@pytest.mark.parametrize("backend,scheme,curve_id", [on("emu", "g16", 0), on("emu", "gm17", 1), on("gpu", "g16", 0), on("gpu", "gm17", 1), on("gpu", "g16", 2)])
def test_same_proofs(contexts, backend, scheme, curve_id):
    ctx = context(contexts, backend)
    r = CURVE[curve_id].r
    params, st = proving_program(r)
    b = Built(ctx, curve_id, params, st, return_count=2)
    tox = synth.toxic_waste(curve_id)
    raw = native.setup_gm17(ctx, b.cs, (tox[0], tox[1], tox[2], tox[4])) if scheme == "gm17" else native.setup_g16(ctx, b.cs, tox)
    pk = native.ProvingKey(ctx, curve_id, raw, scheme=scheme)
    rnd = random.Random(0x6B + curve_id)
    rows = [[rnd.randrange(r), rnd.randrange(256), rnd.randrange(r), 1 + rnd.randrange(r - 1), rnd.randrange(r)] for _ in range(2)]
    rr = [(0x1111 * (i + 1), 7 + i, 0x2222 * (i + 3)) if scheme == "gm17" else (0x1111 * (i + 1), 0x2222 * (i + 3)) for i in range(2)]
    prove = lambda a, x: native.prove_gm17(ctx, pk, b.cs, a, *x) if scheme == "gm17" else native.prove_g16_resident(ctx, pk, b.cs, a, *x)
    one = b.run(rows, want_files=False, want_inputs=False)
    with tuned(ctx, exec_wide=1, exec_wide_min=4):
        wide = b.run(rows, want_files=False, want_inputs=False)
        assert ctx.exec_last() == expected_last(b, len(rows), wide_min=4) and ctx.exec_last()[2] > 1
    want = [prove(a, x) for a, x in zip(one.assignments, rr)]
    assert len(set(want)) == 2 and [prove(a, x) for a, x in zip(wide.assignments, rr)] == want
    zs = [to_bytes(b.z(w, row)) for (w, _), row in zip(b.reference(rows), rows)]
    host = native.prove_gm17 if scheme == "gm17" else native.prove_g16
    assert [host(ctx, pk, b.cs, z, *x) for z, x in zip(zs, rr)] == want
    one.close()
    wide.close()
    pk.close()
    b.close()


# ------------------------------------------------------------------ 7. the interface
@pytest.mark.parametrize("backend", BACKENDS)
def test_interface(contexts, backend):
    from oracle import cpu, groth16 as g16
    ctx = context(contexts, backend)
    r = BN254.r
    # counted by hand: level 1 the two arguments; level 2 the first define and the check on the argument, and 70 more defines that
    # make it the widest; level 3 the directive (it reads the first define); level 4 the define that reads the directive's output
    st = [C([(1, 1)], [(2, 1)], [(10, 1)]), C([(1, 1)], ONE, [(1, 1)]), D([([(10, 1)], ONE)], [11, 12], "ConditionEq"), C([(11, 1)], [(2, 1)], [(13, 1)])]
    st += [C([(1, 1)], [(2, 1), (0, k)], [(100 + k, 1)]) for k in range(70)]
    b = Built(ctx, 0, [(1, True), (2, False)], st)
    assert b.plan.levels() == (4, 72, 76, 3)
    L = ctx.lib.L
    out = np.zeros(4, dtype=np.uint64)
    assert L.zkhip_xplan_levels(None, native._ptr(out)) == BAD_ARG and L.zkhip_xplan_levels(b.plan.h, None) == BAD_ARG
    assert L.zkhip_exec_last(None, native._ptr(out)) == BAD_ARG and L.zkhip_exec_last(ctx.h, None) == BAD_ARG
    fresh = native.Context(0, ctx.lib)
    assert fresh.exec_last() == (0, 0, 0, 0)
    fresh.close()
    for value in (-1, (1 << 20) + 1):
        with pytest.raises(native.ZkhipError) as e:
            ctx.tune("exec_wide_min", value)
        assert e.value.code == BAD_ARG
    for value in (-1, 2):
        with pytest.raises(native.ZkhipError) as e:
            ctx.tune("exec_wide", value)
        assert e.value.code == BAD_ARG
    ctx.tune("exec_wide_min", 1 << 20)
    ctx.tune("exec_wide_min", 0)
    both_routes(ctx, b, [[3, 4], [0, 1]], wide_min=64)
    assert ctx.exec_last() == (2, 1, 3, 64)      # a run (2), the level of 72, a run (1, 1)
    b.close()
    # allowed under an open queue, refused under a pending split proof (and the two read-only calls are not)
    params, pst = proving_program(r)
    b = Built(ctx, 0, params, pst, return_count=2)
    rnd = random.Random(0x52)
    rows = [[rnd.randrange(r), rnd.randrange(256), rnd.randrange(r), 1 + rnd.randrange(r - 1), rnd.randrange(r)] for _ in range(3)]
    ref = b.reference(rows)
    one = b.run(rows)
    pk = native.ProvingKey(ctx, 0, native.setup_g16(ctx, b.cs, synth.toxic_waste(0)))
    rr = [(0x1111 * (i + 1), 0x2222 * (i + 3)) for i in range(3)]
    want = [native.prove_g16(ctx, pk, b.cs, to_bytes(b.z(w, row)), *x) for (w, _), row, x in zip(ref, rows, rr)]
    ctx.tune("exec_wide", 1)
    try:
        with native.ProofQueue(ctx, pk, b.cs) as q:
            q.submit(to_bytes(b.z(ref[0][0], rows[0])), rr[0])
            got = b.run(rows)
            assert ctx.exec_last() == expected_last(b, len(rows))
            same(got, one)
            q.submit(got.assignments[1], rr[1])
            q.submit(got.assignments[2], rr[2])
            assert [q.collect()[1] for _ in range(3)] == want
            got.close()
        pk.close()
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
        assert b.plan.levels()[2] == b.plan.n_args + b.plan.n_statements and ctx.exec_last()[0] == 2      # read-only: allowed
        assert native.prove_g16_split_end(ctx, spk, cs, other).tobytes() == part.tobytes()
        assert b.run(rows).files == one.files and ctx.exec_last()[0] == 2
        spk.close()
        cs.close()
    finally:
        ctx.tune("exec_wide", 0)
    one.close()
    b.close()


def cli_checks(tmp_path, lib, exe, env):
    """`compute-witness --wide` writes the file of `compute-witness`; `generate-proof --arguments .. --wide` the proof.json without"""
    ctx = native.Context(0, lib)
    r = BN254.r
    params, st = proving_program(r)
    b = Built(ctx, 0, params, st, return_count=2, plan=False)
    paths = {k: str(tmp_path / k) for k in ("out", "proving.key", "witness", "witness.wide", "proof.json", "proof.wide.json")}
    open(paths["out"], "wb").write(b.data.tobytes())
    native.setup_g16(ctx, b.cs, synth.toxic_waste(0)).tofile(paths["proving.key"])
    row = [12345678901234567890123, 201, r - 1, 77, 1 << 64]
    w, bad = b.reference([row])[0]
    assert bad is None
    args = [str(v) for v in row]
    run = lambda *a: subprocess.run([exe] + list(a), capture_output=True, text=True, cwd=ROOT, env=env)
    plain = run("compute-witness", "-i", paths["out"], "-o", paths["witness"], "--verbose", "-a", *args)
    wide = run("compute-witness", "-i", paths["out"], "-o", paths["witness.wide"], "--verbose", "--wide", "-a", *args)
    assert plain.returncode == 0 and wide.returncode == 0, plain.stderr + wide.stderr
    assert open(paths["witness.wide"], "rb").read() == open(paths["witness"], "rb").read() == ir.serialize_witness(w)
    assert wide.stdout == plain.stdout.replace(paths["witness"], paths["witness.wide"])
    common = ["generate-proof", "-i", paths["out"], "-p", paths["proving.key"], "--entropy", "e", "-s", "g16"]
    one = run(*common, "-j", paths["proof.json"], "--arguments", *args)
    two = run(*common, "-j", paths["proof.wide.json"], "--wide", "--arguments", *args)
    assert one.returncode == 0 and two.returncode == 0, one.stderr + two.stderr
    assert open(paths["proof.json"], "rb").read() == open(paths["proof.wide.json"], "rb").read()
    # a failing check is named the same way
    failing = serde_model.program_file(r, [X.parameter(1, True)], [C([(1, 1)], [(1, 1)], [(2, 1)]), C([(2, 1)], [(0, 1)], [(0, 9)])], 0)
    open(paths["out"], "wb").write(failing)
    out = run("compute-witness", "-i", paths["out"], "-o", paths["witness"], "--wide", "-a", "4")
    assert out.returncode == 1 and "Execution failed: statement 1 of the program (constraint 1) is not satisfied" in out.stderr
    b.close()
    ctx.close()


def test_cli_wide_on_emulator(tmp_path):
    from emu_util import EMU_LIB, emu_library
    cli_checks(tmp_path, emu_library(), os.path.join(HERE, "_emu", "zkhip-cli-emu"), dict(os.environ, ZKHIP_LIBRARY=EMU_LIB))


@GPU
def test_cli_wide_on_gpu(tmp_path):
    cli_checks(tmp_path, native.default_library(), os.path.join(ROOT, "zokrates_amd", "zkhip-cli"), os.environ)


# ------------------------------------------------------------------ 8. the schedule on the host, alone
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "asan-ubsan"])
def test_level_schedule_stand_alone(tmp_path, flags):
    """tests/host/exec_levels.cpp: xplan.h's schedule over hand-written and seeded random streams — every instruction once, the
    three hazard rules for every pair that shares a slot, minimal levels, and the store of a shuffled level-by-level execution against
    the store of stream order (the opcode bodies of wexec.cuh over host field arithmetic)"""
    exe = str(tmp_path / "exec_levels")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DZK_EMU"] + list(flags) +
                          ["-I", os.path.join(ROOT, "zokrates_amd", "csrc"), "-x", "c++", os.path.join(HERE, "host", "exec_levels.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 failures"), out.stdout + out.stderr
