"""The C ABI called OUT of its intended order.  Every kernel is held to the oracle and every entry point is tested in the order it was
written for; the one stateful pair of the ABI — zkhip_prove_g16_split_begin / _end, which leaves a proof PENDING across two calls — is
held here to its contract (include/zkhip.h, Conventions): while a proof is pending the context refuses, on the host and without
touching the proof, every call that could reach its buffers, its streams or its key; `end` finishes the proof of ITS begin and only
that; `abort` drops it.

  a. named sequences (SEQUENCES): one contract each;
  b. a seeded random walk over both contexts against an explicit model (Model), which must visit every (operation, state) pair of its
     legality table three times;
  c. two contexts driven from two host threads at once (GPU only: the fibre emulator is one process-wide scheduler — csrc/emu.h
     `emu::G()` — and cannot run two launches at a time; the members of a zkhip_multi run one after the other there for the same reason).

Every expected proof is the oracle's closed form (cpu.trapdoor / cpu.gm17_trapdoor); every expected refusal is a ZkhipError carrying
ZKHIP_ERR_BAD_ARG.  The unmarked tests run the kernel sources on the TEST-ONLY emulator, the `gpu` ones the same functions on the
device — there also at n = 3000, where the MSMs have real slices and the B list is thinned.  State tests, not size tests."""
import random
import threading
import time

import numpy as np
import pytest

from oracle import cpu
from zokrates_amd import native, synth

from emu_util import emu_library

BAD_ARG, UNSATISFIED = -1, -5
R_BN254 = synth.FR_MODULUS[0]


def _le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


class Case:
    """One constraint system with its keys (oracle setup), a pool of (witness, r, s) triples and what the oracle says they prove to."""

    def __init__(self, curve_id, n, seed, triples=12, gm17=True):
        self.curve_id, self.n = curve_id, n
        self.circ = synth.circuit(curve_id, n=n, kind="sha", seed=seed)
        self.mats = self.circ.mats()
        self.oc = cpu.Circuit.from_csr(curve_id, n, self.circ.l, self.circ.w, self.mats)
        tox = synth.toxic_waste(curve_id, seed ^ 0x70C5)
        self.tb = _le(tox)
        self.raw = cpu.ProvingKey.setup(self.oc, self.tb).serialize()
        rnd = random.Random(seed)
        r_mod = (1 << 252) - 1
        self.zs = [self.circ.assignment(seed + 1 + k) for k in range(3)]
        edge = [(0, 0, 0), (1, 1, 0), (2, 0, 1)]
        self.triples = ([(k % 3, rnd.randrange(r_mod), rnd.randrange(r_mod)) for k in range(9)] + edge)[:triples]
        self.want = [cpu.trapdoor(self.oc, self.tb, self.zs[w], r, s) for w, r, s in self.triples]
        assert len(set(self.want)) == len(self.want)
        # one assignment that does NOT satisfy the system: the variable of the first boolean row b (b - 1) = 0 set to 2
        self.z_bad = np.array(self.zs[0], copy=True)
        assert self.circ.boolean.any()
        self.bad_row = int(np.argmax(self.circ.boolean))
        self.z_bad[32 * (4 + self.bad_row)] = 2
        if gm17:
            t4 = (tox[0], tox[1], tox[2], tox[4])
            self.tb17 = _le(t4)
            self.raw17 = cpu.Gm17ProvingKey.setup(self.oc, self.tb17).serialize()
            self.want17 = [cpu.gm17_trapdoor(self.oc, self.tb17, self.zs[w], r, s) for w, r, s in self.triples[:9]]      # (d1, d2, r) = (r, 7, s)

    def system(self, ctx):
        return native.ConstraintSystem(ctx, self.curve_id, self.n, self.circ.l, self.circ.w, self.mats)


class Rank:
    pass


class Rig:
    """Two contexts as the two ranks of a sharded prover (test_bound_key.split_entry_point_checks), each with: the constraint system,
    its shard S of the key bound from the key file, the WHOLE key W, a GM17 key G, resident assignments — and a second, larger system
    cs2 (n = 61) with an unbound shard U of ITS key.  Computed once, in the intended order, and left unchanged: every witness's two
    halves and every triple's two partial records (canonical, so equal sums are equal bytes)."""

    def __init__(self, lib, n):
        self.lib, self.n = lib, n
        self.case = Case(0, n, 0x5EED0C00 + n)
        self.other = Case(0, 61, 0x5EED0C61, triples=1, gm17=False)
        cs_ = self.case
        self.ranks = []
        for k in range(2):
            rk = Rank()
            rk.k = k
            rk.ctx = native.Context(0, lib)
            rk.cs = cs_.system(rk.ctx)
            rk.S = native.ProvingKey(rk.ctx, 0, cs_.raw, rank=k, world=2)
            rk.S.bind_shard(rk.cs, cs_.raw)
            rk.W = native.ProvingKey(rk.ctx, 0, cs_.raw)
            rk.G = native.ProvingKey(rk.ctx, 0, cs_.raw17, scheme="gm17")
            rk.za = [native.Assignment(rk.ctx, rk.cs, z) for z in cs_.zs]
            rk.za_bad = native.Assignment(rk.ctx, rk.cs, cs_.z_bad)
            rk.cs2 = self.other.system(rk.ctx)
            rk.U = native.ProvingKey(rk.ctx, 0, self.other.raw, rank=k, world=2)
            self.ranks.append(rk)
        self.halves = []
        for w in range(len(cs_.zs)):
            i = [t[0] for t in cs_.triples].index(w)
            hv = [self.begin(k, i) for k in range(2)]
            parts = [self.end(k, hv[1 - k]) for k in range(2)]
            assert self.combine(0, parts, i) == cs_.want[i]
            self.halves.append(hv)
        self.parts = []
        for i, (w, r, s) in enumerate(cs_.triples):
            parts = [native.prove_g16_partial(rk.ctx, rk.S, rk.cs, cs_.zs[w], r, s) for rk in self.ranks]
            assert self.combine(1, parts, i) == cs_.want[i]
            self.parts.append(parts)

    # ---- the calls, by rank and triple
    def begin(self, k, i, key=None, system=None, half=None, r=None, resident=False):
        rk, (w, r0, s) = self.ranks[k], self.case.triples[i]
        z = self.other.zs[0] if system is rk.cs2 else rk.za[w] if resident else self.case.zs[w]
        return native.prove_g16_split_begin(rk.ctx, key or rk.S, system or rk.cs, z, r0 if r is None else r, s, k if half is None else half)

    def end(self, k, other_half, key=None, system=None):
        rk = self.ranks[k]
        return native.prove_g16_split_end(rk.ctx, key or rk.S, system or rk.cs, other_half)

    def abort(self, k):
        native.prove_g16_split_abort(self.ranks[k].ctx)

    def combine(self, k, parts, i):
        rk, (_, r, s) = self.ranks[k], self.case.triples[i]
        return native.combine_g16(rk.ctx, rk.S, parts, r, s)

    def split_both(self, i, between=None):
        """begin on both ranks, `between()`, end on both, the combined proof."""
        hv = [self.begin(k, i) for k in range(2)]
        if between:
            between()
        parts = [self.end(k, hv[1 - k]) for k in range(2)]
        return self.combine(0, parts, i)

    def lone(self, k, i):
        rk, (w, r, s) = self.ranks[k], self.case.triples[i]
        return native.prove_g16(rk.ctx, rk.W, rk.cs, self.case.zs[w], r, s)

    def observe(self, k):
        """What a refused call must leave as it was: which key is bound to which system, and the checked mode."""
        rk = self.ranks[k]
        return (rk.W.is_bound(rk.cs), rk.S.is_bound(rk.cs), rk.G.is_bound(rk.cs), rk.U.is_bound(rk.cs2), rk.ctx.set_checked(None))

    def last_error(self, k):
        return self.lib.L.zkhip_last_error(self.ranks[k].ctx.h).decode()

    def refused(self, k, call, pending):
        """`call` is refused with ZKHIP_ERR_BAD_ARG, says why, and changes nothing; while a proof is pending the message names it."""
        before = self.observe(k)
        with pytest.raises(native.ZkhipError) as e:
            call()
        assert e.value.code == BAD_ARG, str(e.value)
        msg = self.last_error(k)
        assert msg, "a refusal without a message"
        if pending:
            assert "split proof" in msg and "pending" in msg, msg
        assert self.observe(k) == before
        return msg

    def reset(self):
        """Back to the state __init__ left (also after a failed test): nothing pending, S bound, W and G as loaded, checked off."""
        for rk in self.ranks:
            native.prove_g16_split_abort(rk.ctx)
            rk.ctx.set_checked(False)
            rk.ctx.tune("slots", 3)
            rk.ctx.tune("serial", 0)
            if rk.W.is_bound(rk.cs):
                rk.W.unbind()
            if not rk.S.is_bound(rk.cs):
                rk.S.bind_shard(rk.cs, self.case.raw)

    def close(self):
        for rk in self.ranks:
            native.prove_g16_split_abort(rk.ctx)
            for h in [rk.S, rk.W, rk.G, rk.U, rk.za_bad] + rk.za:
                h.close()
            rk.ctx.close()


# ------------------------------------------------------------------ a. named sequences
def seq_unbind(rig):
    """begin, unbind -> refused; end gives the right record: with the partner's it is the oracle's proof."""
    rk = rig.ranks[0]
    assert rig.split_both(0, lambda: rig.refused(0, rk.S.unbind, True)) == rig.case.want[0]
    assert rk.S.is_bound(rk.cs)
    rk.W.bind(rk.cs)      # ... nor any other key of that context
    assert rig.split_both(1, lambda: rig.refused(0, rk.W.unbind, True)) == rig.case.want[1]
    assert rk.W.is_bound(rk.cs)


def seq_bind(rig):
    """begin, bind / bind_shard -> refused; end is right."""
    rk = rig.ranks[1]

    def between():
        rig.refused(1, lambda: rk.W.bind(rk.cs), True)
        rig.refused(1, lambda: rk.S.bind_shard(rk.cs, rig.case.raw), True)
        rig.refused(1, lambda: rk.U.bind_shard(rk.cs2, rig.other.raw), True)
    assert rig.split_both(2, between) == rig.case.want[2]
    assert not rk.W.is_bound(rk.cs) and not rk.U.is_bound(rk.cs2)


def seq_begin_twice(rig):
    """begin, begin -> refused; end is right (the proof of the FIRST begin)."""
    assert rig.split_both(3, lambda: rig.refused(0, lambda: rig.begin(0, 4), True)) == rig.case.want[3]


def seq_prove_calls(rig):
    """begin, then every prove call and r1cs_check on the same context -> all refused; end is right."""
    rk, cs_ = rig.ranks[0], rig.case
    w, r, s = cs_.triples[5]
    z, za = cs_.zs[w], rk.za[w]

    def between():
        rig.refused(0, lambda: native.prove_g16(rk.ctx, rk.W, rk.cs, z, r, s), True)
        rig.refused(0, lambda: native.prove_g16_resident(rk.ctx, rk.W, rk.cs, za, r, s), True)
        rig.refused(0, lambda: native.prove_g16_resident_batch(rk.ctx, rk.W, rk.cs, [za] * 3, [(r, s)] * 3), True)
        rig.refused(0, lambda: native.prove_g16_batch(rk.ctx, rk.W, rk.cs, np.concatenate([z] * 2), [(r, s)] * 2), True)
        rig.refused(0, lambda: native.prove_g16_partial(rk.ctx, rk.S, rk.cs, z, r, s), True)
        rig.refused(0, lambda: rk.cs.check(z), True)
        rig.refused(0, lambda: rk.cs.check(za), True)
        rig.refused(0, lambda: native.prove_gm17(rk.ctx, rk.G, rk.cs, z, r, 7, s), True)
        rig.refused(0, lambda: native.prove_gm17(rk.ctx, rk.G, rk.cs, za, r, 7, s), True)
        rig.refused(0, lambda: native.prove_gm17_partial(rk.ctx, rk.G, rk.cs, z, r, 7, s), True)
    assert rig.split_both(4, between) == cs_.want[4]
    assert rig.lone(0, 5) == cs_.want[5]


def seq_tune_and_checked(rig):
    """begin, tune(serial, 1) -> refused, set_checked(1) -> refused; end is right."""
    rk = rig.ranks[0]

    def between():
        rig.refused(0, lambda: rk.ctx.tune("serial", 1), True)
        rig.refused(0, lambda: rk.ctx.tune("slots", 2), True)
        rig.refused(0, lambda: rk.ctx.set_checked(True), True)
        rig.refused(0, lambda: rk.ctx.set_checked(False), True)
        assert rk.ctx.set_checked(None) is False          # (reporting is not changing)
    assert rig.split_both(6, between) == rig.case.want[6]


def seq_end_alone_and_twice(rig):
    """end without begin -> refused; begin, end, end -> the second end refused; the next ordinary proof is right."""
    cs_ = rig.case
    fresh = native.Context(0, rig.lib)
    try:
        cs = cs_.system(fresh)
        sh = native.ProvingKey(fresh, 0, cs_.raw, rank=0, world=2)
        sh.bind_shard(cs, cs_.raw)
        with pytest.raises(native.ZkhipError) as e:
            native.prove_g16_split_end(fresh, sh, cs, rig.halves[0][1])
        assert e.value.code == BAD_ARG and rig.lib.L.zkhip_last_error(fresh.h)
        sh.close()
    finally:
        fresh.close()
    hv = [rig.begin(k, 7) for k in range(2)]
    parts = [rig.end(k, hv[1 - k]) for k in range(2)]
    assert rig.combine(0, parts, 7) == cs_.want[7]
    for k in range(2):
        rig.refused(k, lambda: rig.end(k, hv[1 - k]), False)
    assert rig.lone(0, 8) == cs_.want[8] and rig.lone(1, 0) == cs_.want[0]
    parts = [native.prove_g16_partial(rk.ctx, rk.S, rk.cs, cs_.zs[cs_.triples[7][0]], *cs_.triples[7][1:]) for rk in rig.ranks]
    assert rig.combine(1, parts, 7) == cs_.want[7]


def seq_end_with_other_handles(rig):
    """begin(pk, cs), end(pk2, cs2) of a second, LARGER system on the same context -> refused; end(pk, cs2) -> refused; end(pk, cs) is right."""
    rk = rig.ranks[0]
    big = np.zeros((rk.U.hlen + 1) * 32, dtype=np.uint8)
    if rig.n < rig.other.n:      # (the n = 29 rig: a copy of the other key's N x 32 bytes would not fit the pending proof's vectors)
        assert big.size > rig.halves[0][0].size

    def between():
        rig.refused(0, lambda: rig.end(0, big, key=rk.U, system=rk.cs2), True)
        rig.refused(0, lambda: rig.end(0, rig.halves[0][1], system=rk.cs2), True)
        rig.refused(0, lambda: rig.end(0, big, key=rk.U), True)
    assert rig.split_both(8, between) == rig.case.want[8]


def seq_abort(rig):
    """begin, abort: prove, partial, bind / unbind and a fresh begin .. end all work and are right; abort with nothing pending is OK."""
    cs_ = rig.case
    rig.abort(0)                                         # nothing pending
    hv = [rig.begin(k, 9) for k in range(2)]
    rig.abort(0)
    rig.refused(0, lambda: rig.end(0, hv[1]), False)     # dropped: nothing to end
    rk = rig.ranks[0]
    assert rig.lone(0, 10) == cs_.want[10]
    w, r, s = cs_.triples[11]
    assert bytes(native.prove_g16_partial(rk.ctx, rk.S, rk.cs, cs_.zs[w], r, s)) == bytes(rig.parts[11][0])
    rk.W.bind(rk.cs)
    assert rig.lone(0, 10) == cs_.want[10]
    rk.W.unbind()
    rk.S.unbind()
    rk.S.bind_shard(rk.cs, cs_.raw)
    assert rig.begin(0, 9).tobytes() == hv[0].tobytes()      # a fresh begin .. end on the aborted rank; its partner is still pending
    parts = [rig.end(0, hv[1]), rig.end(1, hv[0])]
    assert rig.combine(0, parts, 9) == cs_.want[9]
    rig.abort(0)
    rig.abort(1)
    assert rig.split_both(2) == cs_.want[2]


def seq_refused_begin(rig):
    """A begin refused for its ARGUMENTS leaves nothing pending: a non-canonical r, an unbound key, half = 2; the next proof works."""
    rk, cs_ = rig.ranks[0], rig.case
    for call in (lambda: rig.begin(0, 0, r=R_BN254),
                 lambda: rig.begin(0, 0, r=(1 << 256) - 1),
                 lambda: rig.begin(0, 0, key=rk.U, system=rk.cs2),
                 lambda: rig.begin(0, 0, key=rk.W),
                 lambda: rig.begin(0, 0, half=2),
                 lambda: rig.begin(0, 0, half=-1)):
        rig.refused(0, call, False)
        rig.refused(0, lambda: rig.end(0, rig.halves[0][1]), False)      # nothing is pending
        assert rig.lone(0, 1) == cs_.want[1]
    assert rig.split_both(0) == cs_.want[0]


SEQUENCES = {f.__name__[4:]: f for f in (seq_unbind, seq_bind, seq_begin_twice, seq_prove_calls, seq_tune_and_checked, seq_end_alone_and_twice,
                                         seq_end_with_other_handles, seq_abort, seq_refused_begin)}


# ------------------------------------------------------------------ b. the walk and its model
IDLE, PENDING = "idle", "pending"
#        operation            legal in            weight when idle, when pending
TABLE = {
    "lone_host":        ((IDLE,),          1, 1),
    "lone_resident":    ((IDLE,),          1, 1),
    "batch_resident":   ((IDLE,),          1, 1),
    "batch_host":       ((IDLE,),          1, 1),
    "gm17":             ((IDLE,),          1, 1),
    "partial":          ((IDLE,),          1, 1),
    "check":            ((IDLE,),          1, 1),
    "checked_bad":      ((IDLE,),          1, 1),
    "bind":             ((IDLE,),          1, 1),
    "unbind":           ((IDLE,),          1, 1),
    "rebind_shard":     ((IDLE,),          1, 1),
    "export_import":    ((IDLE,),          1, 1),
    "checked_on":       ((IDLE,),          1, 1),
    "checked_off":      ((IDLE,),          1, 1),
    "tune_slots":       ((IDLE,),          1, 1),
    "begin":            ((IDLE,),         2, 1),
    "end":              ((PENDING,),       1, 1),
    "abort":            ((IDLE, PENDING),  1, 1),
    "combine":          ((IDLE, PENDING),  1, 1),
    "begin_half2":      ((),               1, 1),      # the deliberately illegal ones
    "begin_bad_r":      ((),               1, 1),
    "begin_unbound":    ((),               1, 1),
    "end_other_key":    ((),               1, 1),
    "end_other_cs":     ((),               1, 1),
}
# (the seed was searched for, on the model alone, among 3000: the walk's coverage condition is a condition on it — test_the_walk_is_a_function_of_its_seed)
WALK_SEED, WALK_STEPS, MIN_VISITS = 792395, 300, 3


class Model:
    """What the contract says the two contexts are after every call.  Per context: the pending proof (triple, or None), the checked mode,
    the slot count; per key: bound or not.  It draws the walk (a function of the seed alone) and names every call's expected class."""

    def __init__(self, seed, n_triples):
        self.rnd = random.Random(seed)
        self.n_triples = n_triples
        self.pending = [None, None]
        self.checked = [False, False]
        self.w_bound = [False, False]
        self.visits = {(op, st): 0 for op in TABLE for st in (IDLE, PENDING)}

    def state(self, k):
        return IDLE if self.pending[k] is None else PENDING

    def draw(self):
        """(context, operation, its arguments, expected class: "ok" / "refused")"""
        k = self.rnd.randrange(2)
        st = self.state(k)
        ops = list(TABLE)
        op = self.rnd.choices(ops, weights=[TABLE[o][1 if st == IDLE else 2] for o in ops])[0]
        args = {"i": self.rnd.randrange(self.n_triples), "j": self.rnd.randrange(9), "count": self.rnd.choice([2, 3]), "slots": self.rnd.randrange(1, 5),
                "resident": self.rnd.random() < 0.5}
        self.visits[(op, st)] += 1
        return k, op, args, "ok" if st in TABLE[op][0] else "refused"

    def apply(self, k, op, args):
        """a LEGAL call's effect on the state (a refused one has none)"""
        if op == "begin":
            self.pending[k] = args["i"]
        elif op in ("end", "abort"):
            self.pending[k] = None
        elif op == "bind":
            self.w_bound[k] = True
        elif op in ("unbind", "export_import"):
            self.w_bound[k] = False
        elif op == "checked_on":
            self.checked[k] = True
        elif op == "checked_off":
            self.checked[k] = False

    def expect(self, k):
        return (self.w_bound[k], True, False, False, self.checked[k])      # (Rig.observe)


def do_step(rig, model, k, op, a):
    """One legal call (or group of calls that make one operation) of the walk, every proof it returns held to the oracle."""
    rk, cs_ = rig.ranks[k], rig.case
    i, j = a["i"], a["j"]
    w, r, s = cs_.triples[i]
    if op == "lone_host":
        assert native.prove_g16(rk.ctx, rk.W, rk.cs, cs_.zs[w], r, s) == cs_.want[i]
    elif op == "lone_resident":
        assert native.prove_g16_resident(rk.ctx, rk.W, rk.cs, rk.za[w], r, s) == cs_.want[i]
    elif op in ("batch_resident", "batch_host"):
        idx = [(i + q) % len(cs_.triples) for q in range(a["count"])]
        if op == "batch_resident":
            proofs, _ = native.prove_g16_resident_batch(rk.ctx, rk.W, rk.cs, [rk.za[cs_.triples[q][0]] for q in idx], [cs_.triples[q][1:] for q in idx])
        else:
            proofs, _ = native.prove_g16_batch(rk.ctx, rk.W, rk.cs, np.concatenate([cs_.zs[cs_.triples[q][0]] for q in idx]), [cs_.triples[q][1:] for q in idx])
        assert proofs == [cs_.want[q] for q in idx]
    elif op == "gm17":
        wj, rj, sj = cs_.triples[j]
        assert native.prove_gm17(rk.ctx, rk.G, rk.cs, rk.za[wj] if a["resident"] else cs_.zs[wj], rj, 7, sj) == cs_.want17[j]
    elif op == "partial":
        part = native.prove_g16_partial(rk.ctx, rk.S, rk.cs, rk.za[w] if a["resident"] else cs_.zs[w], r, s)
        assert bytes(part) == bytes(rig.parts[i][k])
        parts = [part, rig.parts[i][1 - k]]
        assert rig.combine(k, parts if k == 0 else parts[::-1], i) == cs_.want[i]
    elif op == "check":
        assert rk.cs.check(cs_.zs[w]) == (None, 0)
        assert rk.cs.check(rk.za_bad) == (cs_.bad_row, 1)
    elif op == "checked_bad":
        # the one unsatisfying assignment of the pool, in checked mode: ZKHIP_ERR_UNSATISFIED, a zero-filled slot, a usable context
        rk.ctx.set_checked(True)
        with pytest.raises(native.ZkhipError) as e:
            native.prove_g16_resident_batch(rk.ctx, rk.W, rk.cs, [rk.za[w], rk.za_bad], [(r, s), (r, s)])
        assert e.value.code == UNSATISFIED and [u[0] for u in e.value.unsatisfied] == [1]
        assert e.value.proofs == [cs_.want[i], bytes(len(cs_.want[i]))]
        with pytest.raises(native.ZkhipError) as e:
            native.prove_g16(rk.ctx, rk.W, rk.cs, cs_.z_bad, r, s)
        assert e.value.code == UNSATISFIED and rig.last_error(k)
        assert native.prove_g16(rk.ctx, rk.W, rk.cs, cs_.zs[w], r, s) == cs_.want[i]
        rk.ctx.set_checked(model.checked[k])
    elif op == "bind":
        rk.W.bind(rk.cs)
    elif op == "unbind":
        rk.W.unbind()
    elif op == "rebind_shard":
        rk.S.unbind()
        assert not rk.S.is_bound(rk.cs)
        rk.S.bind_shard(rk.cs, cs_.raw)
    elif op == "export_import":
        image = rk.W.export_image()
        rk.W.close()
        rk.W = native.ProvingKey.from_image(rk.ctx, 0, image)
    elif op == "checked_on":
        rk.ctx.set_checked(True)
    elif op == "checked_off":
        rk.ctx.set_checked(False)
    elif op == "tune_slots":
        rk.ctx.tune("slots", a["slots"])
    elif op == "begin":
        half = rig.begin(k, i, resident=a["resident"])
        assert half.tobytes() == rig.halves[w][k].tobytes()
    elif op == "end":
        p = model.pending[k]
        part = rig.end(k, rig.halves[cs_.triples[p][0]][1 - k])
        assert bytes(part) == bytes(rig.parts[p][k])
        parts = [part, rig.parts[p][1 - k]]
        assert rig.combine(k, parts if k == 0 else parts[::-1], p) == cs_.want[p]
    elif op == "abort":
        rig.abort(k)
    elif op == "combine":
        assert rig.combine(k, rig.parts[i], i) == cs_.want[i]
    else:
        raise AssertionError(op)


def illegal_call(rig, model, k, op, a):
    """The call of `op` the table says is refused in this state (for a group of calls: the first one)."""
    rk, cs_ = rig.ranks[k], rig.case
    i = a["i"]
    w, r, s = cs_.triples[i]
    other_half = rig.halves[w][1 - k]
    return {
        "lone_host": lambda: native.prove_g16(rk.ctx, rk.W, rk.cs, cs_.zs[w], r, s),
        "lone_resident": lambda: native.prove_g16_resident(rk.ctx, rk.W, rk.cs, rk.za[w], r, s),
        "batch_resident": lambda: native.prove_g16_resident_batch(rk.ctx, rk.W, rk.cs, [rk.za[w]] * a["count"], [(r, s)] * a["count"]),
        "batch_host": lambda: native.prove_g16_batch(rk.ctx, rk.W, rk.cs, np.concatenate([cs_.zs[w]] * a["count"]), [(r, s)] * a["count"]),
        "gm17": lambda: native.prove_gm17(rk.ctx, rk.G, rk.cs, cs_.zs[w], r, 7, s),
        "partial": lambda: native.prove_g16_partial(rk.ctx, rk.S, rk.cs, cs_.zs[w], r, s),
        "check": lambda: rk.cs.check(cs_.zs[w]),
        "checked_bad": lambda: rk.ctx.set_checked(True),
        "bind": lambda: rk.W.bind(rk.cs),
        "unbind": lambda: rk.W.unbind(),
        "rebind_shard": lambda: rk.S.unbind(),
        "export_import": lambda: rk.W.export_image(),
        "checked_on": lambda: rk.ctx.set_checked(True),
        "checked_off": lambda: rk.ctx.set_checked(False),
        "tune_slots": lambda: rk.ctx.tune("slots", a["slots"]),
        "begin": lambda: rig.begin(k, i),
        "end": lambda: rig.end(k, other_half),
        "begin_half2": lambda: rig.begin(k, i, half=2),
        "begin_bad_r": lambda: rig.begin(k, i, r=R_BN254 + 5),
        "begin_unbound": lambda: rig.begin(k, i, key=rk.U, system=rk.cs2),
        "end_other_key": lambda: rig.end(k, np.zeros((rk.U.hlen + 1) * 32, dtype=np.uint8), key=rk.U, system=rk.cs2),
        "end_other_cs": lambda: rig.end(k, other_half, system=rk.cs2),
    }[op]


def walk(rig, steps=WALK_STEPS, seed=WALK_SEED):
    model = Model(seed, len(rig.case.triples))
    for step in range(steps):
        k, op, a, cls = model.draw()
        st = model.state(k)
        try:
            if cls == "ok":
                do_step(rig, model, k, op, a)
                model.apply(k, op, a)
            else:
                rig.refused(k, illegal_call(rig, model, k, op, a), st == PENDING)
            assert rig.observe(k) == model.expect(k)
        except BaseException as e:
            raise AssertionError("step %d: %s on context %d (%s, expected %s): %s" % (step, op, k, st, cls, e)) from e
    # whatever is still pending ends right: no refused call has touched it
    for k in range(2):
        if model.pending[k] is not None:
            do_step(rig, model, k, "end", {"i": 0, "j": 0})
            model.apply(k, "end", {})
    return model


def coverage_table(model):
    lines = ["%-16s %6s %8s   (legal in: idle / pending)" % ("operation", "idle", "pending")]
    for op in TABLE:
        lines.append("%-16s %6d %8d   %s / %s" % (op, model.visits[(op, IDLE)], model.visits[(op, PENDING)],
                                                   "ok" if IDLE in TABLE[op][0] else "refused", "ok" if PENDING in TABLE[op][0] else "refused"))
    return "\n".join(lines)


def walk_checks(rig):
    model = walk(rig)
    print(coverage_table(model))
    short = {pair: v for pair, v in model.visits.items() if v < MIN_VISITS}
    assert not short, "the walk's seed must visit every (operation, state) pair %d times: %r" % (MIN_VISITS, short)


# ------------------------------------------------------------------ the emulator half
@pytest.fixture(scope="module")
def emu_rig():
    rig = Rig(emu_library(), 29)
    assert "EMULATOR" in rig.ranks[0].ctx.describe()
    yield rig
    rig.close()


@pytest.fixture
def rig(emu_rig):
    yield emu_rig
    emu_rig.reset()


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_sequence(rig, name):
    SEQUENCES[name](rig)


def test_walk_against_the_model(rig):
    walk_checks(rig)


def test_the_walk_is_a_function_of_its_seed():
    """The coverage condition is a property of (seed, weights, steps): the model alone, no library."""
    model = Model(WALK_SEED, 12)
    for _ in range(WALK_STEPS):
        k, op, a, cls = model.draw()
        if cls == "ok":
            model.apply(k, op, a)
    assert min(model.visits.values()) >= MIN_VISITS, coverage_table(model)


# ------------------------------------------------------------------ the gpu half
@pytest.fixture(scope="module", params=[29, 3000], ids=lambda n: "n%d" % n)
def gpu_rig(request):
    rig = Rig(native.default_library(), request.param)
    d = rig.ranks[0].ctx.describe()
    assert "gfx950" in d and "EMULATOR" not in d, d
    yield rig
    rig.close()


@pytest.fixture
def grig(gpu_rig):
    yield gpu_rig
    gpu_rig.reset()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_gpu_sequence(grig, name):
    SEQUENCES[name](grig)


@pytest.mark.gpu
def test_gpu_walk_against_the_model(grig):
    walk_checks(grig)


# ------------------------------------------------------------------ c. two contexts, two host threads
CALLS_PER_THREAD = 24
# The bound under test is "does not deadlock", not speed: 20 x the time the two workloads below take one after the other in ONE thread
# on the emulator build — 21.0 s + 11.0 s = 32.0 s (profiles/call_sequences_checks.txt) —, which is itself far slower than the device.
THREAD_JOIN_TIMEOUT_S = 20 * 32.0


class Workload:
    """One thread's context, key and expected results (all from the oracle, computed before the threads start) and its seeded mix of
    CALLS_PER_THREAD calls of four kinds: lone proofs from HOST memory (the staging ring every context of a device shares), resident
    batches of 3, zkhip_ntt at 2^11, zkhip_msm_g1 over 1000 points."""

    def __init__(self, lib, curve_id, n, bound, seed):
        self.case = c = Case(curve_id, n, seed, triples=6, gm17=False)
        self.curve_id = curve_id
        self.ctx = native.Context(0, lib)
        self.describe = self.ctx.describe()
        self.cs = c.system(self.ctx)
        self.pk = native.ProvingKey(self.ctx, curve_id, c.raw)
        if bound:
            self.pk.bind(self.cs)
        self.za = [native.Assignment(self.ctx, self.cs, z) for z in c.zs]
        rnd = np.random.default_rng(seed)
        self.ntt_in = rnd.integers(0, 256, size=(1 << 11) * 32, dtype=np.uint8)
        self.ntt_in.reshape(-1, 32)[:, 31] &= 0x0f
        self.ntt_want = {d: cpu.ntt(curve_id, self.ntt_in, d).tobytes() for d in ("fft", "coset_ifft")}
        nb = native.FQ_BYTES[curve_id]
        off = 2 * nb + 3 * 4 * nb + 8 + c.circ.l * 2 * nb + 2 * 2 * nb + 8      # a_query of the key file: m >= 1000 points
        assert c.circ.m >= 1000
        self.bases = np.array(c.raw[off:off + 1000 * 2 * nb], copy=True)
        self.scalars = rnd.integers(0, 256, size=1000 * 32, dtype=np.uint8)
        self.scalars.reshape(-1, 32)[:, 31] &= 0x0f
        self.msm_want = cpu.msm(curve_id, 1, self.bases, self.scalars)
        mix = random.Random(seed)
        self.calls = [(mix.choice(["lone_host", "batch_resident", "ntt", "msm"]), mix.randrange(len(c.triples))) for _ in range(CALLS_PER_THREAD)]
        for q, kind in enumerate(["lone_host", "batch_resident", "ntt", "msm"]):      # every kind at least once, wherever the seed put the others
            self.calls[q * 5] = (kind, self.calls[q * 5][1])
        self.failures = []

    def run(self, barrier=None):
        c = self.case
        try:
            if barrier is not None:
                barrier.wait(timeout=60)
            for q, (kind, i) in enumerate(self.calls):
                w, r, s = c.triples[i]
                if kind == "lone_host":
                    ok = native.prove_g16(self.ctx, self.pk, self.cs, c.zs[w], r, s) == c.want[i]
                elif kind == "batch_resident":
                    idx = [(i + d) % len(c.triples) for d in range(3)]
                    proofs, _ = native.prove_g16_resident_batch(self.ctx, self.pk, self.cs, [self.za[c.triples[d][0]] for d in idx], [c.triples[d][1:] for d in idx])
                    ok = proofs == [c.want[d] for d in idx]
                elif kind == "ntt":
                    d = ("fft", "coset_ifft")[i & 1]
                    ok = self.ctx.ntt(self.curve_id, self.ntt_in, d).tobytes() == self.ntt_want[d]
                else:
                    ok = self.ctx.msm(self.curve_id, 1, self.bases, self.scalars) == self.msm_want
                if not ok:
                    self.failures.append("call %d (%s, triple %d) differs from the oracle" % (q, kind, i))
        except BaseException as e:      # (collected: asserted in the main thread)
            self.failures.append("%s: %s" % (type(e).__name__, e))

    def close(self):
        for h in [self.pk] + self.za:
            h.close()
        self.ctx.close()


def make_workloads(lib):
    return [Workload(lib, 0, 3000, True, 0x5EED0CA0), Workload(lib, 1, 1000, False, 0x5EED0CB0)]


def thread_checks(lib):
    loads = make_workloads(lib)
    barrier = threading.Barrier(2)
    threads = [threading.Thread(target=ld.run, args=(barrier,), daemon=True) for ld in loads]
    try:
        t0 = time.perf_counter()
        for t in threads:
            t.start()
        deadline = t0 + THREAD_JOIN_TIMEOUT_S
        for t in threads:
            t.join(timeout=max(0.0, deadline - time.perf_counter()))
        stuck = [q for q, t in enumerate(threads) if t.is_alive()]
        print("two threads, %d calls each: %.2f s" % (CALLS_PER_THREAD, time.perf_counter() - t0))
        assert not stuck, "thread(s) %r still running after %.0f s: a deadlock between two contexts of one device" % (stuck, THREAD_JOIN_TIMEOUT_S)
        assert loads[0].failures == [] and loads[1].failures == []
    finally:
        if not any(t.is_alive() for t in threads):
            for ld in loads:
                ld.close()


@pytest.mark.gpu
def test_gpu_two_contexts_two_host_threads():
    """`distinct contexts may be used from distinct threads` (zkhip.h): thread A proves BN254 at n = 3000 over a bound key, thread B
    BLS12-381 at n = 1000 over an unbound one, started together; what they share is process-wide — the device's staging ring and the
    allocation table of csrc/devrt.h.  Every result is compared with the oracle inside its thread."""
    thread_checks(native.default_library())
