"""The proof queue (zkhip_queue_*): up to ctx->nslots proofs in flight ACROSS calls — the pipeline of the *_batch calls with the caller
as the loop — held to its contract (include/zkhip.h, Conventions):

  1. parity across slot reuse: 2 x capacity + 1 proofs in the steady-state order, Groth16 and GM17, bound and unbound key, the three
     witness sources mixed in one queue, every proof byte for byte;
  2. three call orders, the same bytes, zkhip_queue_state right after every call;
  3. full (ZKHIP_ERR_BUSY) and empty (ZKHIP_ERR_BAD_ARG), neither disturbing what is in flight;
  4. buffer ownership: z, packed and rnd overwritten as soon as submit returns;
  5. failures of ONE proof fail that ticket only; a refused submit consumes no ticket;
  6. the pending rule: an open queue refuses what a pending split proof refuses, and names itself;
  7. a seeded random walk against an explicit model (a FIFO of expected proofs plus the capacity);
  8. GPU only: two contexts with a queue each on two host threads; twelve proofs under ZKHIP_TUNE_STREAM_JITTER;
  9. the compiled host layer: Hip::open_queue against Hip::prove with equal StdRng seeds (tests/host/proof_queue.cpp).

Every expected proof is the oracle's closed form (cpu.trapdoor / cpu.gm17_trapdoor).  State tests, like test_call_sequences.py, with
that file's cases and sizes: the unmarked half runs the kernel sources on the TEST-ONLY emulator, the `gpu` half the same functions
on the device — there at n = 3000, where the MSMs have real slices and the B list is thinned."""
import ctypes as C
import os
import random
import re
import subprocess
import threading
import time

import numpy as np
import pytest

from oracle import cpu
from zokrates_amd import native, synth

from emu_util import EMU_DIR, emu_library
from test_call_sequences import Case, _le

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, PARSE, DEVICE, UNSATISFIED, BUSY = -1, -2, -4, -5, -6
KINDS = ("host", "resident", "packed")
NOT_CANONICAL = "not a canonical field element"


def staging_chunk_bytes():
    """StagingRing::CHUNK of csrc/devrt.h: the unit in which a host buffer travels through the library's pinned ring."""
    text = open(os.path.join(ROOT, "zokrates_amd", "csrc", "devrt.h")).read()
    m = re.search(r"static constexpr size_t CHUNK = \(size_t\)(\d+) << (\d+);", text)
    assert m, "StagingRing::CHUNK has moved"
    return int(m.group(1)) << int(m.group(2))


class QRig:
    """One context with a constraint system, its Groth16 key W and GM17 key G (oracle setup), the pool of Case — every witness as host
    bytes, resident and packed — and what goes wrong for ONE proof: an assignment that does not satisfy the system, one with an entry
    equal to r (host and packed), and a resident assignment of another system."""

    def __init__(self, lib, n, curve_id=0, gm17=True, other=True):
        self.lib, self.n, self.curve_id = lib, n, curve_id
        self.case = c = Case(curve_id, n, 0x5EED9000 + 16 * n + curve_id, gm17=gm17)
        self.ctx = native.Context(0, lib)
        self.cs = c.system(self.ctx)
        self.W = native.ProvingKey(self.ctx, curve_id, c.raw)
        self.G = native.ProvingKey(self.ctx, curve_id, c.raw17, scheme="gm17") if gm17 else None
        self.za = [native.Assignment(self.ctx, self.cs, z) for z in c.zs]
        self.zp = [native.pack_assignment(z, lib) for z in c.zs]
        self.za_bad = native.Assignment(self.ctx, self.cs, c.z_bad)
        r_mod = synth.FR_MODULUS[curve_id]
        self.z_r = np.array(c.zs[1], copy=True)
        self.z_r[-32:] = np.frombuffer(int(r_mod).to_bytes(32, "little"), dtype=np.uint8)      # the last witness variable = r
        # (the packer has no curve and refuses only what is canonical in NO field: r of BN254 packs, r of BLS12-381 — the largest — does not)
        self.zp_r = native.pack_assignment(self.z_r, lib) if curve_id == 0 else None
        self.other = self.cs2 = self.za2 = None
        if other:
            self.other = Case(curve_id, 61, 0x5EED9061, triples=1, gm17=False)
            self.cs2 = self.other.system(self.ctx)
            self.za2 = native.Assignment(self.ctx, self.cs2, self.other.zs[0])
        self.queues = []

    def key(self, scheme, bound):
        pk = self.G if scheme == "gm17" else self.W
        if bound != pk.is_bound(self.cs):
            pk.bind(self.cs) if bound else pk.unbind()
        return pk

    def rnd(self, scheme, i):
        _, r, s = self.case.triples[i]
        return (r, 7, s) if scheme == "gm17" else (r, s)

    def want(self, scheme, i):
        return self.case.want17[i] if scheme == "gm17" else self.case.want[i]

    def last_error(self):
        return self.lib.L.zkhip_last_error(self.ctx.h).decode()

    def open(self, scheme="g16", bound=False):
        d = Driver(self, scheme, bound)
        self.queues.append(d)
        return d

    def reset(self):
        """Back to the state __init__ left (also after a failed test): no queue, no split proof, checked off, three slots, keys unbound."""
        for d in self.queues:
            d.q.close()
        self.queues = []
        native.prove_g16_split_abort(self.ctx)
        self.ctx.set_checked(False)
        self.ctx.tune("slots", 3)
        for pk in (self.W, self.G):
            if pk is not None and pk.is_bound(self.cs):
                pk.unbind()

    def close(self):
        for d in self.queues:
            d.q.close()
        for h in [self.W, self.G, self.za_bad, self.za2] + self.za:
            if h is not None:
                h.close()
        self.ctx.close()


class Driver:
    """A queue and the model of it: the FIFO of what it must return, the capacity, the next ticket.  Every call is followed by a look
    at zkhip_queue_state.  A FIFO entry is (ticket, expected proof bytes) or (ticket, (error code, part of the message))."""

    def __init__(self, rig, scheme="g16", bound=False):
        self.rig, self.scheme = rig, scheme
        self.q = native.ProofQueue(rig.ctx, rig.key(scheme, bound), rig.cs)
        self.cap = self.q.state()[0]
        self.fifo, self.next = [], 0
        self.look()

    def look(self):
        assert self.q.state() == (self.cap, len(self.fifo)), (self.q.state(), self.cap, len(self.fifo))

    def source(self, kind, w):
        rig = self.rig
        return {"host": rig.case.zs[w], "resident": rig.za[w], "packed": rig.zp[w]}[kind]

    def submit(self, kind, i):
        """triple i of the pool from the source `kind`"""
        return self.submit_raw(kind, self.source(kind, self.rig.case.triples[i][0]), self.rig.rnd(self.scheme, i), self.rig.want(self.scheme, i))

    def submit_raw(self, kind, z, rnd, want):
        t = self.q.submit_packed(z, rnd) if kind == "packed" else self.q.submit(z, rnd)
        assert t == self.next, (t, self.next)
        self.next += 1
        self.fifo.append((t, want))
        self.look()
        return t

    def collect(self):
        t, want = self.fifo.pop(0)
        if isinstance(want, tuple):
            with pytest.raises(native.ZkhipError) as e:
                self.q.collect()
            assert e.value.code == want[0] and want[1] in str(e.value) and e.value.ticket == t, (str(e.value), want, t)
            self.look()
            return e.value
        got = self.q.collect()
        assert got[0] == t, (got[0], t)
        assert got[1] == want, "ticket %d differs from the oracle" % t
        self.look()
        return got[1]

    def drain(self):
        while self.fifo:
            self.collect()

    def refused(self, call, code, part=""):
        """`call` fails with `code`, says why, and changes nothing of the queue: not what is in flight, not the next ticket"""
        with pytest.raises(native.ZkhipError) as e:
            call()
        assert e.value.code == code and part in str(e.value), (str(e.value), code, part)
        assert self.rig.last_error(), "a refusal without a message"
        self.look()
        return str(e.value)

    def close(self):
        self.q.close()
        self.fifo = []
        if self in self.rig.queues:
            self.rig.queues.remove(self)


def steady(d, proofs):
    """submit, submit, submit, collect, submit, collect ...: run_batch's own schedule; `proofs` = [(kind, triple)]"""
    for kind, i in proofs:
        if len(d.fifo) == d.cap:
            d.collect()
        d.submit(kind, i)
    d.drain()


# ------------------------------------------------------------------ 1. parity across slot reuse
def parity_checks(rig, scheme, bound):
    d = rig.open(scheme, bound)
    total = 2 * d.cap + 1
    # (the source moves on by one per round of the slots, so that every slot sees more than one kind)
    steady(d, [(KINDS[(k + k // d.cap) % 3], k % 9) for k in range(total)])
    assert d.next == total
    d.close()


# ------------------------------------------------------------------ 2. call orders
def order_checks(rig):
    proofs = [(KINDS[k % 3], (2 * k + 1) % 9) for k in range(7)]
    d = rig.open()
    # fill to capacity, then drain
    for lo in range(0, len(proofs), d.cap):
        for kind, i in proofs[lo:lo + d.cap]:
            d.submit(kind, i)
        d.drain()
    # strictly one in flight
    for kind, i in proofs:
        d.submit(kind, i)
        d.collect()
    # the steady state
    steady(d, proofs)
    assert d.next == 3 * len(proofs)
    d.close()


# ------------------------------------------------------------------ 3. full and empty
def full_and_empty_checks(rig):
    d = rig.open()
    d.refused(d.q.collect, BAD_ARG, "empty")
    for k in range(d.cap):
        d.submit(KINDS[k % 3], k)
    for kind in KINDS:
        msg = d.refused(lambda: d.q.submit_packed(rig.zp[0], rig.rnd("g16", 0)) if kind == "packed" else d.q.submit(d.source(kind, 0), rig.rnd("g16", 0)), BUSY)
        assert "collect" in msg
    d.collect()
    d.submit("host", 8)                      # the ticket the refused submits did not take
    d.drain()
    d.refused(d.q.collect, BAD_ARG, "empty")
    assert d.q.ready() is False
    d.submit("resident", 4)
    d.collect()
    d.close()


# ------------------------------------------------------------------ 4. buffer ownership
class OneKey:
    """what a Driver needs of a rig, for a case that has one key and no pool"""

    def __init__(self, lib, ctx, cs, pk):
        self.lib, self.ctx, self.cs, self.pk, self.queues = lib, ctx, cs, pk, []

    def key(self, scheme, bound):
        return self.pk


def ownership_checks(d, zs, packed, rnds, wants):
    """every host buffer of a submit — z, packed, rnd — is overwritten with 0xff as soon as the call returns; rnds: uint8 arrays"""
    for k, want in enumerate(wants):
        if len(d.fifo) == d.cap:
            d.collect()
        rb = np.array(rnds[k], copy=True)
        if k % 2:
            buf = np.array(packed[k], copy=True)
            d.submit_raw("packed", buf, rb, want)
        else:
            buf = np.array(zs[k], copy=True)
            d.submit_raw("host", buf, rb, want)
        buf[:] = 0xff
        rb[:] = 0xff
    d.drain()
    d.close()


def small_ownership_checks(rig):
    c = rig.case
    idx = list(range(2 * 3 + 1))
    rnds = [np.frombuffer(_le(rig.rnd("g16", i)), dtype=np.uint8) for i in idx]
    ownership_checks(rig.open(), [c.zs[c.triples[i][0]] for i in idx], [rig.zp[c.triples[i][0]] for i in idx], rnds, [c.want[i] for i in idx])


# ------------------------------------------------------------------ 5. failures of one proof
def one_proof_fails_checks(rig):
    c = rig.case
    # (a) in checked mode the middle ticket does not satisfy the system: row named, slot zeroed, one triple with proof index 0
    for bad in (c.z_bad, rig.za_bad):
        rig.ctx.set_checked(True)
        d = rig.open()
        assert d.cap == 3
        d.submit("packed", 0)
        d.submit_raw("host", bad, rig.rnd("g16", 1), (UNSATISFIED, "constraint %d of %d" % (c.bad_row, c.n)))
        d.submit("resident", 2)
        d.collect()
        e = d.collect()
        assert e.unsatisfied == [(0, c.bad_row, 1)] and e.proofs == [bytes(len(c.want[0]))] and "ticket 1" in str(e)
        d.submit("host", 3)                  # into the slot of the ticket that failed
        d.drain()
        d.close()
        rig.ctx.set_checked(False)
    # (b) an entry equal to r, from host memory; (c) the same assignment packed (a 32-byte value >= r): found on the device, told at collect
    for scheme in ("g16", "gm17"):
        for kind, z in (("host", rig.z_r), ("packed", rig.zp_r)):
            d = rig.open(scheme)
            d.submit("resident", 4)
            d.submit_raw(kind, z, rig.rnd(scheme, 5), (BAD_ARG, NOT_CANONICAL))
            d.submit("host", 6)
            d.drain()
            d.submit(kind, 7)
            d.submit("packed", 8)
            d.drain()
            d.close()


def refused_submit_checks(rig, scheme):
    """every submit that is refused for its ARGUMENTS consumes no ticket and leaves what is in flight as it was"""
    c, L = rig.case, rig.lib.L
    r_mod = synth.FR_MODULUS[rig.curve_id]
    # what zkhip_assignment_upload_packed says about the same malformed buffers (asked before the queue is open: uploads are refused under it)
    bad_magic = np.array(rig.zp[0], copy=True)
    bad_magic[0] ^= 1
    malformed = [rig.zp[0][:-16], bad_magic, rig.zp[0][:24]]
    said = []
    for buf in malformed:
        with pytest.raises(native.ZkhipError) as e:
            native.Assignment.from_packed(rig.ctx, rig.cs, buf)
        assert e.value.code == PARSE
        said.append(str(e.value))
    d = rig.open(scheme)
    d.submit("host", 0)
    d.submit("packed", 1)
    rnd = np.frombuffer(_le(rig.rnd(scheme, 2)), dtype=np.uint8)
    z, za = c.zs[0], rig.za[0]
    ticket = C.c_uint64()

    def raw(zp, zh):
        rig.ctx._check(L.zkhip_queue_submit(d.q.h, zp, zh, native._ptr(rnd), C.byref(ticket)))
    d.refused(lambda: raw(None, None), BAD_ARG, "exactly one")
    d.refused(lambda: raw(native._ptr(z), za.h), BAD_ARG, "exactly one")
    d.refused(lambda: rig.ctx._check(L.zkhip_queue_submit(d.q.h, native._ptr(z), None, None, C.byref(ticket))), BAD_ARG, "null")
    d.refused(lambda: rig.ctx._check(L.zkhip_queue_submit_packed(d.q.h, None, 0, native._ptr(rnd), C.byref(ticket))), BAD_ARG, "null")
    z_two = np.array(z, copy=True)
    z_two[0] = 2
    d.refused(lambda: d.q.submit(z_two, rnd), BAD_ARG, "z[0] must be 1")
    d.refused(lambda: d.q.submit_packed(native.pack_assignment(z_two, rig.lib), rnd), BAD_ARG, "z[0] must be 1")
    for k in range(len(rnd) // 32):          # every blinding scalar in turn: r itself, and all ones
        for v in (r_mod, (1 << 256) - 1):
            bad = np.array(rnd, copy=True)
            bad[32 * k:32 * k + 32] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
            for kind, src in (("host", z), ("resident", za), ("packed", rig.zp[0])):
                d.refused(lambda: d.q.submit_packed(src, bad) if kind == "packed" else d.q.submit(src, bad), BAD_ARG, NOT_CANONICAL)
    d.refused(lambda: d.q.submit(rig.za2, rnd), BAD_ARG, "does not match")
    d.refused(lambda: d.q.submit_packed(native.pack_assignment(rig.other.zs[0], rig.lib), rnd), BAD_ARG, "elements")
    for buf, msg in zip(malformed, said):
        assert d.refused(lambda: d.q.submit_packed(buf, rnd), PARSE) == msg
    d.submit("resident", 2)                  # ticket 2: none was consumed
    d.drain()
    d.close()


# ------------------------------------------------------------------ 6. the pending rule
def pending_rule_checks(rig):
    c, ctx, cs = rig.case, rig.ctx, rig.cs
    w, r, s = c.triples[3]
    z, za = c.zs[w], rig.za[w]
    S = native.ProvingKey(ctx, rig.curve_id, c.raw, rank=0, world=2)
    S.bind_shard(cs, c.raw)
    try:
        with pytest.raises(native.ZkhipError) as e:      # whole keys only
            native.ProofQueue(ctx, S, cs)
        assert e.value.code == BAD_ARG and "shard" in str(e.value)
        # a queue is not opened over a pending split proof: that rule's own message
        native.prove_g16_split_begin(ctx, S, cs, z, r, s, 0)
        with pytest.raises(native.ZkhipError) as e:
            native.ProofQueue(ctx, rig.W, cs)
        assert e.value.code == BAD_ARG and "split proof" in str(e.value) and "pending" in str(e.value)
        native.prove_g16_split_abort(ctx)

        d = rig.open()
        d.submit("host", 0)
        d.submit("packed", 1)
        ntt_in = np.zeros(32 << 4, dtype=np.uint8)
        nb = native.FQ_BYTES[rig.curve_id]
        families = {
            "prove": lambda: native.prove_g16(ctx, rig.W, cs, z, r, s),
            "prove_resident": lambda: native.prove_g16_resident(ctx, rig.W, cs, za, r, s),
            "prove_batch": lambda: native.prove_g16_resident_batch(ctx, rig.W, cs, [za] * 2, [(r, s)] * 2),
            "prove_gm17": lambda: native.prove_gm17(ctx, rig.G, cs, z, r, 7, s),
            "prove_partial": lambda: native.prove_g16_partial(ctx, S, cs, z, r, s),
            "r1cs_check": lambda: cs.check(z),
            "bind": lambda: rig.W.bind(cs),
            "unbind": lambda: rig.W.unbind(),
            "tune": lambda: ctx.tune("slots", 2),
            "set_checked_on": lambda: ctx.set_checked(True),
            "set_checked_off": lambda: ctx.set_checked(False),
            "key_load": lambda: native.ProvingKey(ctx, rig.curve_id, c.raw),
            "key_export": lambda: rig.W.export_image(),
            "upload": lambda: native.Assignment(ctx, cs, z),
            "upload_packed": lambda: native.Assignment.from_packed(ctx, cs, rig.zp[w]),
            "ntt": lambda: ctx.ntt(rig.curve_id, ntt_in, "fft"),
            "msm_g1": lambda: ctx.msm(rig.curve_id, 1, np.zeros(2 * nb, dtype=np.uint8), np.zeros(32, dtype=np.uint8)),
            "split_begin": lambda: native.prove_g16_split_begin(ctx, S, cs, z, r, s, 0),
            "second_open": lambda: native.ProofQueue(ctx, rig.W, cs),
        }
        before = (rig.W.is_bound(cs), ctx.set_checked(None))
        for name, call in families.items():
            msg = d.refused(call, BAD_ARG)
            assert "proof queue" in msg and "open" in msg, (name, msg)
        assert (rig.W.is_bound(cs), ctx.set_checked(None)) == before
        # the calls the rule lets through
        assert ctx.set_checked(None) is False and ctx.unsatisfied() == [] and "zkhip" in ctx.describe()
        rig.W._dims()
        assert native.partial_size(ctx, rig.curve_id) > 0
        assert native.unpack_assignment(rig.zp[w], rig.lib).tobytes() == z.tobytes()
        native.prove_g16_split_abort(ctx)                 # nothing to drop, nothing dropped
        d.look()
        d.refused(lambda: native.prove_g16_split_end(ctx, S, cs, np.zeros((S.hlen + 1) * 32, dtype=np.uint8)), BAD_ARG, "no split proof pending")
        d.submit("resident", 2)
        d.drain()
        # close with two proofs uncollected: the context is an ordinary context again
        d.submit("host", 4)
        d.submit("resident", 5)
        d.close()
        assert native.prove_g16(ctx, rig.W, cs, z, r, s) == c.want[3]
        assert native.prove_gm17(ctx, rig.G, cs, za, r, 7, s) == c.want17[3]
        ctx.tune("slots", 2)                              # capacity is the slot count when the queue is opened
        d = rig.open()
        assert d.cap == 2
        steady(d, [(KINDS[k % 3], k) for k in range(5)])
        d.close()
    finally:
        native.prove_g16_split_abort(ctx)
        S.close()


# ------------------------------------------------------------------ 7. the walk and its model
EMPTY, PARTIAL, FULL = "empty", "partial", "full"
STATES = (EMPTY, PARTIAL, FULL)
#        operation          legal in                 weight when empty, partial, full
Q_TABLE = {
    "submit_host":     ((EMPTY, PARTIAL),        3, 3, 1),
    "submit_resident": ((EMPTY, PARTIAL),        3, 3, 1),
    "submit_packed":   ((EMPTY, PARTIAL),        3, 3, 1),
    "collect":         ((PARTIAL, FULL),         1, 2, 3),
    "ready":           ((EMPTY, PARTIAL, FULL),  1, 1, 1),
    "reopen":          ((EMPTY, PARTIAL, FULL),  1, 1, 1),
    "foreign":         ((),                      1, 1, 1),      # a call of another family: always refused, names the queue
}
# (the seed was searched for, on the model alone, among 400: the coverage condition is a condition on it — test_the_queue_walk_is_a_function_of_its_seed)
Q_WALK_SEED, Q_WALK_STEPS, Q_MIN_VISITS, Q_CAP = 19, 300, 3, 3


class QModel:
    """What the contract says the queue is after every call: how many proofs are in flight (the FIFO itself is the Driver's).  It draws
    the walk — a function of the seed alone — and names every call's expected class."""

    def __init__(self, seed, cap=Q_CAP):
        self.rnd = random.Random(seed)
        self.cap, self.n = cap, 0
        self.visits = {(op, st): 0 for op in Q_TABLE for st in STATES}

    def state(self):
        return EMPTY if self.n == 0 else FULL if self.n == self.cap else PARTIAL

    def draw(self):
        st = self.state()
        ops = list(Q_TABLE)
        op = self.rnd.choices(ops, weights=[Q_TABLE[o][1 + STATES.index(st)] for o in ops])[0]
        args = {"i": self.rnd.randrange(9), "scheme": self.rnd.choice(["g16", "gm17"]), "bound": self.rnd.random() < 0.5, "foreign": self.rnd.randrange(4)}
        self.visits[(op, st)] += 1
        return op, args, "ok" if st in Q_TABLE[op][0] else "refused"

    def apply(self, op):
        if op.startswith("submit"):
            self.n += 1
        elif op == "collect":
            self.n -= 1
        elif op == "reopen":
            self.n = 0


def queue_walk(rig, steps=Q_WALK_STEPS, seed=Q_WALK_SEED):
    model = QModel(seed)
    d = rig.open()
    assert d.cap == model.cap
    emulated = "EMULATOR" in rig.ctx.describe()
    c, ctx, cs = rig.case, rig.ctx, rig.cs
    for step in range(steps):
        op, a, cls = model.draw()
        st = model.state()
        try:
            if op.startswith("submit"):
                kind = op[7:]
                if cls == "ok":
                    d.submit(kind, a["i"])
                else:
                    d.refused(lambda: d.q.submit_packed(rig.zp[0], rig.rnd(d.scheme, 0)) if kind == "packed" else d.q.submit(d.source(kind, 0), rig.rnd(d.scheme, 0)), BUSY)
            elif op == "collect":
                if cls == "ok":
                    d.collect()
                else:
                    d.refused(d.q.collect, BAD_ARG, "empty")
            elif op == "ready":
                got = d.q.ready()
                assert got is False if st == EMPTY else got in (True, False)
                if emulated and st != EMPTY:
                    assert got is True
                d.look()
            elif op == "reopen":                     # whatever is in flight is dropped; the next queue counts from 0
                d.close()
                d = rig.open(a["scheme"], a["bound"])
            else:
                w, r, s = c.triples[a["i"]]
                call = (lambda: native.prove_g16(ctx, rig.W, cs, c.zs[w], r, s), lambda: ctx.tune("serial", 1), lambda: cs.check(rig.za[w]),
                        lambda: native.ProofQueue(ctx, rig.G, cs))[a["foreign"]]
                assert "proof queue" in d.refused(call, BAD_ARG)
            if cls == "ok":
                model.apply(op)
            assert len(d.fifo) == model.n
        except BaseException as e:
            raise AssertionError("step %d: %s (%s, expected %s): %s" % (step, op, st, cls, e)) from e
    d.drain()      # whatever is still in flight comes out right: no refused call has touched it
    d.close()
    return model


def q_coverage_table(model):
    lines = ["%-16s %6s %8s %6s" % (("operation",) + STATES)]
    for op in Q_TABLE:
        lines.append("%-16s %6d %8d %6d   legal in: %s" % ((op,) + tuple(model.visits[(op, st)] for st in STATES) + (", ".join(Q_TABLE[op][0]) or "-",)))
    return "\n".join(lines)


def queue_walk_checks(rig):
    model = queue_walk(rig)
    print(q_coverage_table(model))
    short = {pair: v for pair, v in model.visits.items() if v < Q_MIN_VISITS}
    assert not short, "the walk's seed must visit every (operation, state) pair %d times: %r" % (Q_MIN_VISITS, short)


def test_the_queue_walk_is_a_function_of_its_seed():
    """The coverage condition is a property of (seed, weights, steps): the model alone, no library."""
    model = QModel(Q_WALK_SEED)
    for _ in range(Q_WALK_STEPS):
        op, a, cls = model.draw()
        if cls == "ok":
            model.apply(op)
    assert min(model.visits.values()) >= Q_MIN_VISITS, q_coverage_table(model)


CHECKS = {
    "parity_g16": lambda rig: parity_checks(rig, "g16", False),
    "parity_g16_bound": lambda rig: parity_checks(rig, "g16", True),
    "parity_gm17": lambda rig: parity_checks(rig, "gm17", False),
    "parity_gm17_bound": lambda rig: parity_checks(rig, "gm17", True),
    "call_orders": order_checks,
    "full_and_empty": full_and_empty_checks,
    "buffer_ownership": small_ownership_checks,
    "one_proof_fails": one_proof_fails_checks,
    "refused_submits_g16": lambda rig: refused_submit_checks(rig, "g16"),
    "refused_submits_gm17": lambda rig: refused_submit_checks(rig, "gm17"),
    "pending_rule": pending_rule_checks,
    "walk": queue_walk_checks,
}


# ------------------------------------------------------------------ the emulator half
@pytest.fixture(scope="module")
def emu_rig():
    rig = QRig(emu_library(), 29)
    assert "EMULATOR" in rig.ctx.describe()
    yield rig
    rig.close()


@pytest.fixture
def rig(emu_rig):
    yield emu_rig
    emu_rig.reset()


@pytest.mark.parametrize("name", list(CHECKS))
def test_queue(rig, name):
    CHECKS[name](rig)


def test_queue_bls12_381():
    rig = QRig(emu_library(), 29, curve_id=1, other=False)
    try:
        parity_checks(rig, "g16", True)
        parity_checks(rig, "gm17", False)
    finally:
        rig.close()


# ------------------------------------------------------------------ the gpu half
@pytest.fixture(scope="module")
def gpu_rig():
    rig = QRig(native.default_library(), 3000)
    d = rig.ctx.describe()
    assert "gfx950" in d and "EMULATOR" not in d, d
    yield rig
    rig.close()


@pytest.fixture
def grig(gpu_rig):
    yield gpu_rig
    gpu_rig.reset()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CHECKS))
def test_gpu_queue(grig, name):
    CHECKS[name](grig)


@pytest.mark.gpu
def test_gpu_queue_bls12_381():
    rig = QRig(native.default_library(), 1000, curve_id=1, gm17=False, other=False)
    try:
        parity_checks(rig, "g16", True)
    finally:
        rig.close()


def bls12_377_checks(lib, n):
    """The third curve has no C++ oracle: the closed form is tests/bls377_ref.py's (as in test_bls12_377.py), the key the device's."""
    import bls377_ref as ref
    from oracle import formats
    from oracle import groth16 as g16
    curve = ref.CURVE
    cs, z = g16.synthetic_chain(curve, n, 0x377E, "sha")
    zb = np.frombuffer(_le(z), dtype=np.uint8)
    tox = g16.Toxic.from_seed(curve)
    ctx = native.Context(0, lib)
    try:
        ncs = native.ConstraintSystem(ctx, 2, cs.n, cs.l, cs.w, ref.csr(cs))
        pk = native.ProvingKey(ctx, 2, native.setup_g16(ctx, ncs, (tox.alpha, tox.beta, tox.gamma, tox.delta, tox.tau)))
        za, zp = native.Assignment(ctx, ncs, zb), native.pack_assignment(zb, lib)
        rnds = [(0x1234567 + 77 * k, 0x89abcdef0123 + k) for k in range(7)]
        wants = [formats.proof_raw(curve, ref.g16_trapdoor(cs, tox, z, a, b)) for a, b in rnds]
        d = Driver(OneKey(lib, ctx, ncs, pk))
        for k, want in enumerate(wants):
            if len(d.fifo) == d.cap:
                d.collect()
            kind = KINDS[(k + k // d.cap) % 3]
            d.submit_raw(kind, {"host": zb, "resident": za, "packed": zp}[kind], rnds[k], want)
        d.drain()
        d.close()
        pk.close()
    finally:
        ctx.close()


def test_queue_bls12_377():
    bls12_377_checks(emu_library(), 30)


@pytest.mark.gpu
def test_gpu_queue_bls12_377():
    bls12_377_checks(native.default_library(), 1000)


@pytest.mark.gpu
def test_gpu_buffer_ownership_beyond_two_staging_chunks():
    """Test 4 where the copy is long: an assignment of more than TWO chunks of the pinned staging ring (StagingRing::CHUNK, csrc/devrt.h
    — a host buffer travels through the ring chunk by chunk, and submit must have copied the last one before it returns), dense, so
    that its packed form is as long.  The n = 3000 rig above is the case below ONE chunk."""
    chunk = staging_chunk_bytes()
    lib = native.default_library()
    ctx = native.Context(0, lib)
    n = 2 * chunk // 32 + 5000
    circ = synth.circuit(0, n=n, kind="dense", seed=0x5EED9F00)
    assert circ.m * 32 > 2 * chunk
    cs = native.ConstraintSystem(ctx, 0, circ.n, circ.l, circ.w, circ.mats())
    tox = synth.toxic_waste(0, 0x9F00)
    pk = native.ProvingKey(ctx, 0, native.setup_g16(ctx, cs, tox))
    oc = cpu.Circuit.from_csr(0, circ.n, circ.l, circ.w, circ.mats())
    tb = _le(tox)
    zs = [circ.assignment(0x9F01 + k) for k in range(2)]
    zp = [native.pack_assignment(z, lib) for z in zs]
    assert all(p.size > 2 * chunk for p in zp)
    rnds = [(0x1234567 + k, 0x7654321 + 3 * k) for k in range(4)]
    wants = [cpu.trapdoor(oc, tb, zs[k % 2], *rnds[k]) for k in range(4)]
    try:
        ownership_checks(Driver(OneKey(lib, ctx, cs, pk)),[zs[k % 2] for k in range(4)], [zp[k % 2] for k in range(4)], [np.frombuffer(_le(t), dtype=np.uint8) for t in rnds], wants)
    finally:
        pk.close()
        ctx.close()


def test_the_small_rig_is_below_one_staging_chunk():
    """... and what `small_ownership_checks` runs on the device is the other side of that size: one chunk holds its whole assignment."""
    assert (3000 + 4) * 32 < staging_chunk_bytes() and (29 + 4) * 32 < staging_chunk_bytes()


# ------------------------------------------------------------------ 8. two contexts, two host threads; stream jitter
PROOFS_PER_THREAD = 12
# "does not deadlock", not speed: twelve proofs at n = 3000 take well under a second on the device
THREAD_JOIN_TIMEOUT_S = 120.0


class QueueThread:
    def __init__(self, lib, curve_id, n, scheme, bound, seed):
        self.rig = QRig(lib, n, curve_id=curve_id, gm17=scheme == "gm17", other=False)
        self.scheme, self.bound = scheme, bound
        mix = random.Random(seed)
        self.proofs = [(mix.choice(KINDS), mix.randrange(9)) for _ in range(PROOFS_PER_THREAD)]
        self.failures = []

    def run(self, barrier):
        try:
            d = self.rig.open(self.scheme, self.bound)
            barrier.wait(timeout=60)
            steady(d, self.proofs)
            d.close()
        except BaseException as e:      # (collected: asserted in the main thread)
            self.failures.append("%s: %s" % (type(e).__name__, e))


@pytest.mark.gpu
def test_gpu_two_queues_two_host_threads():
    """Two contexts of one device, a queue each, driven from two host threads at once: what they share is process-wide — the staging
    ring and the allocation table of csrc/devrt.h.  Every proof is compared with the oracle inside its thread."""
    lib = native.default_library()
    loads = [QueueThread(lib, 0, 3000, "g16", True, 0x5EED9A00), QueueThread(lib, 0, 1000, "gm17", False, 0x5EED9B00)]
    barrier = threading.Barrier(2)
    threads = [threading.Thread(target=ld.run, args=(barrier,), daemon=True) for ld in loads]
    try:
        t0 = time.perf_counter()
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=max(0.0, t0 + THREAD_JOIN_TIMEOUT_S - time.perf_counter()))
        stuck = [k for k, t in enumerate(threads) if t.is_alive()]
        assert not stuck, "thread(s) %r still running after %.0f s" % (stuck, THREAD_JOIN_TIMEOUT_S)
        assert loads[0].failures == [] and loads[1].failures == []
    finally:
        if not any(t.is_alive() for t in threads):
            for ld in loads:
                ld.rig.close()


@pytest.mark.gpu
def test_gpu_queue_under_stream_jitter(grig):
    """Twelve proofs in the steady state with a random delay in front of every launch and copy: an ordering between two proofs in
    flight that no event carries — the one buffer for packed bytes, a slot reused too early — shows as a wrong proof."""
    grig.ctx.tune("stream_jitter", 300)
    try:
        d = grig.open("g16", True)
        steady(d, [(KINDS[(k + k // 3) % 3], k % 9) for k in range(12)])
        d.close()
    finally:
        grig.ctx.tune("stream_jitter", 0)      # (the knob is process-wide)


# ------------------------------------------------------------------ 9. the compiled host layer
HOST_SRC = os.path.join(ROOT, "tests", "host", "proof_queue.cpp")
BACKEND_SRC = os.path.join(ROOT, "zokrates_amd", "csrc", "host", "backend.cpp")


def host_files(tmp_path, lib):
    """a program, its two keys (device setup over the system as the reader numbers it) and three witnesses, as the files the host layer reads"""
    circ = synth.circuit(0, n=29, kind="sha", seed=0x5EED9C00)
    ids = np.arange(circ.m, dtype=np.int64)
    paths = {"out": tmp_path / "out", "pk": tmp_path / "proving.key", "pk17": tmp_path / "proving17.key"}
    paths["out"].write_bytes(bytes(native.write_program(0, circ.n, circ.m, circ.mats(), ids=ids, library=lib)))
    ctx = native.Context(0, lib)
    prog = native.Program(paths["out"].read_bytes(), lib)
    cs = prog.constraint_system(ctx)
    tox = synth.toxic_waste(0, 0x9C00)
    paths["pk"].write_bytes(bytes(native.setup_g16(ctx, cs, tox)))
    paths["pk17"].write_bytes(bytes(native.setup_gm17(ctx, cs, (tox[0], tox[1], tox[2], tox[4]))))
    cs.close()
    prog.close()
    ctx.close()
    for k in range(3):
        paths["w%d" % k] = tmp_path / ("witness%d" % k)
        paths["w%d" % k].write_bytes(bytes(native.write_witness(ids, circ.assignment(0x9C01 + k))))
    return paths


def host_program_checks(tmp_path, lib, libdir, libname, extra_flags=(), env=None, only=()):
    exe = tmp_path / "proof_queue"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", *extra_flags, HOST_SRC, BACKEND_SRC, "-I" + os.path.join(ROOT, "include"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined", "-o", str(exe)])
    p = host_files(tmp_path, lib)
    out = subprocess.run([str(exe), str(p["out"]), str(p["pk"]), str(p["pk17"]), str(p["w0"]), str(p["w1"]), str(p["w2"]), *only], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "proof queue host checks OK" in out.stdout, out.stdout
    return out.stdout


def test_host_layer_queue_on_emulator(tmp_path):
    """Hip::open_queue: submit / collect against Hip::prove with equal StdRng seeds, plain and compact, both schemes — the stand-alone
    program tests/host/proof_queue.cpp, linked against the emulator build."""
    host_program_checks(tmp_path, emu_library(), EMU_DIR, "zkhip_emu")


def test_host_layer_queue_under_sanitizers(tmp_path):
    """The same stand-alone program, its Groth16 half, with the host layer under AddressSanitizer and UBSan: the program and
    csrc/host/backend.cpp are instrumented, the emulator library is not — so no leak report: the emulator's events are plain `new`s
    that its context never frees, and they are not the host layer's."""
    host_program_checks(tmp_path, emu_library(), EMU_DIR, "zkhip_emu", extra_flags=("-fsanitize=address,undefined", "-fno-omit-frame-pointer"),
                        env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1"), only=("g16",))


@pytest.mark.gpu
def test_gpu_host_layer_queue(tmp_path):
    lib = native.default_library()
    host_program_checks(tmp_path, lib, os.path.dirname(lib.path), "zkhip")
