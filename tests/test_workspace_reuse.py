"""A used context held to the oracle: a call's result does not depend on what the context's workspaces held before the call.

The workspaces of a context only grow (DBuf::ensure, csrc/core.cuh), they are shared by every key, curve, group and scheme that passes
through it, and all-zero memory is the neutral element of nearly everything here: a point at infinity, the scalar 0, an empty bucket.
A kernel that reads a slot nobody wrote is therefore right as long as the slot was fresh, and every other test of the suite runs in
a fresh context or walks its sizes upward.  Two things are done about it here, on the emulator (CPU suite) and on the device (`gpu`)
through the same functions:

  (a) FILLED ALLOCATIONS.  ZKHIP_TUNE_ALLOC_FILL (tests only, process-wide; csrc/devrt.h) makes every device and pinned-host block
      the library allocates come filled with a 32-bit word.  It is set before the test's own context is created and cleared in a
      `finally`.  Every family then runs once at its smallest shapes that still take each code path.  SMALL = 5 on both halves: at
      once a small index or count, a non-zero limb and, repeated, a canonical non-zero Fr — a stale word read as an index, an offset
      or a loop count stays within the first elements of any buffer, which is why it is the only word the device sees.  BYTES =
      0x01010101, every byte non-zero (byte-wide flags), on the emulator alone.
  (b) SHRINKING AND CHANGING SHAPES in one context, fill off, so that what the tails hold is real residue — finite points, canonical
      scalars, counters and offsets of another shape and another element width.  Each sequence first dirties (the larger shape of
      the family, full-width inputs, a batch of nslots + 1 proofs so that every slot's workspaces are grown and written), then
      checks the small shapes.  SEQUENCES names the orders; the `descending_*` ones run every family of the pool from its largest shape to
      its smallest behind three dirtying calls; `walk` is a seeded walk of 40 steps over the whole pool, all curves and both schemes
      mixed, whose conditions — every family directly behind a strictly larger call of its own family (where the pool has one) and
      directly behind a call over another curve or group — are asserted on the model before anything runs; the seed is the first
      for which they hold.

Every expected value comes from a reference: oracle.cpu, tests/bls377_ref.py, tests/exec_ref.py, oracle.ir, or a verdict known by
construction.  Nothing compares the library with itself.  A failing step is named in the assertion (`step <name>`)."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import size_ladder as sl
import test_degenerate_bases as deg
import test_device_exec as dx
import test_device_verify as dv
import test_msm_geometry as geo
import test_proof_queue as pq
import test_witness_device as wd
from emu_util import emu_library
from oracle import cpu
from oracle import groth16 as g16
from oracle.fields import BN254
from test_msm_geometry import case  # noqa: F401  (the module-scoped fixture of the eight geometry cases' data)
from test_size_ladder import EMU_ADHOC_MAX_N, EMU_NTT_MAX, EMU_PROOF_MAX
from zokrates_amd import native

SMALL, BYTES = 0x00000005, 0x01010101
NSLOTS = 3                                  # core.cuh: proofs in flight in the batch calls
NONE = (None, 0)
NAMES = {0: "bn254", 1: "bls12_381", 2: "bls12_377"}


def make_context(backend):
    c = native.Context(0, emu_library()) if backend == "emu" else native.Context(0)
    d = c.describe()
    assert ("EMULATOR" in d) == (backend == "emu") and (backend == "emu" or "gfx950" in d), d
    return c


def set_fill(backend, word):
    """the process-wide word, through a context that lives for this call alone: the test's own context is created after it"""
    c = make_context(backend)
    try:
        c.tune("alloc_fill", word)
    finally:
        c.close()


class Env:
    def __init__(self, backend, ctx, geom):
        self.backend, self.ctx, self.geom = backend, ctx, geom


class Step:
    """One call (or one check function's calls) of the pool.  `size`: a tuple, larger in no component and smaller in one = strictly
    smaller; `first` / `last`: the (curve, group) its first and its last launch run over."""

    def __init__(self, name, family, size, first, run, last=None, backends=("emu", "gpu")):
        self.name, self.family, self.size, self.first, self.last, self.run, self.backends = name, family, tuple(size), first, last or first, run, backends

    def __call__(self, env):
        try:
            self.run(env)
        except AssertionError as e:
            raise AssertionError("step %s: %s" % (self.name, e)) from e

    def __repr__(self):
        return self.name


def larger(a, b):
    """step a is strictly larger than step b of the same family"""
    return a.family == b.family and len(a.size) == len(b.size) and all(x >= y for x, y in zip(a.size, b.size)) and a.size != b.size


# ------------------------------------------------------------------ transforms
def ntt_step(cid, logn, backends=("emu", "gpu")):
    return Step("ntt-%s-2^%d" % (NAMES[cid], logn), "ntt", (logn,), (cid, "fr"), lambda env: sl.check_ntt_rung(env.ctx, cid, logn), backends=backends)


def three_pass(env):
    """2^9 as 2^3 x 2^3 x 2^3 under ntt_max_sublog 4, on the shared context: its plans are dropped on the way in and on the way out"""
    assert sl.ntt_plan(9, sub=4)["passes"] == 3
    try:
        env.ctx.tune("ntt_max_sublog", 4)
        sl.check_ntt(env.ctx, 0, 9)
        sl.check_structured(env.ctx, BN254, 9)
    finally:
        env.ctx.tune("ntt_max_sublog", sl.NTT_MAX_SUBLOG)


# ------------------------------------------------------------------ ad-hoc MSM
MSM_N = 300


def forced_msm(cid, group, c):
    """zkhip_msm over MSM_N points of one group under msm_c: 4 (K = 8: one-level placement) and 9 (K = 256: two-level placement, the
    one-workgroup scan) are the two widths of the ladder that test_msm_geometry.py leaves to it"""
    bits = sl.BITS[cid]
    shape = sl.msm_shape(MSM_N, bits, False, force_c=c)
    assert shape["two_level"] == (c == 9) and shape["sets"] * shape["K"] <= 1 << 17

    def run(env):
        g1, g2, ks, want1, want2 = sl.adhoc_case(cid, c, MSM_N)
        try:
            env.ctx.tune("msm_c", c)
            if group == 1:
                assert env.ctx.msm(cid, 1, g1, ks) == want1
            else:
                assert env.ctx.msm(cid, 2, g2, ks) == want2
        finally:
            env.ctx.tune("msm_c", 0)
    return Step("msm-%s-G%d-c%d" % (NAMES[cid], group, c), "msm", (MSM_N, shape["sets"] * shape["K"]), (cid, group), run)


def geometry_step(name):
    knobs = geo.CASES[name]
    shape = sl.msm_shape(geo.N, sl.BITS[0], False, force_c=knobs["msm_c"])
    return Step("msm-geometry-" + name, "msm", (geo.N, shape["sets"] * shape["K"]), (0, 1), lambda env: geo._run(env.ctx, env.geom, knobs), last=(0, 2))


def degenerate(env):
    """test_degenerate_bases' structured case at width 8, lanes that sit bases at infinity out and lanes that vote: with slices of one
    entry every lane only starts a sum and the fold meets the equal and opposite partial sums; with slices of 2 and 8 a lane's
    (P, -P) pair or run cancels, or its (inf, inf) group adds nothing, ahead of a bucket boundary — slots written by lanes with an
    empty sum"""
    cs = deg.case(0, 1, 360, True)
    cs.check_coverage(8)
    try:
        env.ctx.tune("msm_c", 8)
        for min_slice in (1, 2, 8):
            env.ctx.tune("msm_min_slice", min_slice)
            for mode in (1, 2):
                env.ctx.tune("skip_inf", mode)
                assert env.ctx.msm(0, 1, cs.base_bytes, cs.scalar_bytes) == cs.want, (min_slice, mode)
    finally:
        env.ctx.tune("msm_c", 0)
        env.ctx.tune("msm_min_slice", 8)
        env.ctx.tune("skip_inf", 0)


DEG_SHAPE = sl.msm_shape(360, sl.BITS[0], False, force_c=8)


def dirty_msm_g2(env):
    """the dirtying call of the MSM sequences: G2 of BLS12-381 (the widest Xyzz there is) at the ladder's largest G2 size"""
    n = EMU_ADHOC_MAX_N if env.backend == "emu" else sl.ADHOC_G2_MAX_N
    c = sl.adhoc_window(n, sl.BITS[1])
    g1, g2, ks, want1, want2 = sl.adhoc_case(1, c, n)
    assert env.ctx.msm(1, 2, g2, ks) == want2


def small_msm_g1(env):
    """G1 of BN254 (the narrowest Xyzz) at the width the rule picks for it"""
    c, n = 4, sl.adhoc_rungs(0)[4]
    g1, g2, ks, want1, want2 = sl.adhoc_case(0, c, n)
    assert sl.adhoc_window(n, sl.BITS[0]) == c and env.ctx.msm(0, 1, g1, ks) == want1


# ------------------------------------------------------------------ proofs
def g16_step(cid, L, half=False, backends=("emu", "gpu")):
    return Step("g16-%s-%d%s" % (NAMES[cid], L, "-half" if half else ""), "g16", (sl.synth_dims(L, half)[2], L), (cid, "proof"),
                lambda env: sl.check_g16(env.ctx, cid, L, half), backends=backends)


def gm17_step(cid, L, half=False, backends=("emu", "gpu")):
    return Step("gm17-%s-%d%s" % (NAMES[cid], L, "-half" if half else ""), "gm17", (sl.synth_dims(L, half)[2], L), (cid, "proof"),
                lambda env: sl.check_gm17(env.ctx, cid, L, half), backends=backends)


def batch_rnds(n):
    return [(sl.RS[i % 3][0] + 0x10001 * i, sl.RS[i % 3][1] + 3 * i) for i in range(n)]


def g16_batch(ctx, cid, L, half=False, bound=False, n=NSLOTS + 1):
    """a resident batch of n Groth16 proofs over the oracle's key against the closed form, one by one: with n > nslots every slot's
    workspaces are grown and written"""
    pc = sl.proof_case(cid, L, half)
    cs = native.ConstraintSystem(ctx, cid, pc.n, pc.l, pc.oc.w, pc.mats)
    pk = native.ProvingKey(ctx, cid, cpu.ProvingKey.setup(pc.oc, pc.tb).serialize())
    try:
        if bound:
            pk.bind(cs)
        zas = [native.Assignment(ctx, cs, z) for z in pc.zs]
        rs = batch_rnds(n)
        proofs, _ = native.prove_g16_resident_batch(ctx, pk, cs, [zas[i % 2] for i in range(n)], rs)
        for i in range(n):
            assert proofs[i] == cpu.trapdoor(pc.oc, pc.tb, pc.zs[i % 2], *rs[i]), ("proof %d of the batch" % i, bound)
        for za in zas:
            za.close()
    finally:
        pk.close()
        cs.close()


def gm17_batch(ctx, cid, L, half=False, bound=False, n=NSLOTS + 1):
    pc = sl.proof_case(cid, L, half)
    cs = native.ConstraintSystem(ctx, cid, pc.n, pc.l, pc.oc.w, pc.mats)
    pk = native.ProvingKey(ctx, cid, cpu.Gm17ProvingKey.setup(pc.oc, pc.tb17).serialize(), scheme="gm17")
    try:
        if bound:
            pk.bind(cs)
        zas = [native.Assignment(ctx, cs, z) for z in pc.zs]
        rnds = [(r, 7 + i, s) for i, (r, s) in enumerate(batch_rnds(n))]
        proofs, _ = native.prove_gm17_resident_batch(ctx, pk, cs, [zas[i % 2] for i in range(n)], rnds)
        for i in range(n):
            assert proofs[i] == cpu.gm17_trapdoor(pc.oc, pc.tb17, pc.zs[i % 2], rnds[i][0], rnds[i][2]), ("GM17 proof %d of the batch" % i, bound)
        for za in zas:
            za.close()
    finally:
        pk.close()
        cs.close()


def top_L(backend):
    return EMU_PROOF_MAX[0] if backend == "emu" else 11


# ------------------------------------------------------------------ the sha-like witness
SHA_N = 400


class ShaCase:
    """A sha-like circuit of 400 rows, its oracle key, its witness of bits and a dense assignment (full-width values: it does not
    satisfy the system, the algorithmic oracle says what it proves to)."""

    def __init__(self):
        self.oc = oc = cpu.Circuit.synth(0, SHA_N, 0x5EED0190, "sha")
        self.tb = cpu.toxic_bytes(g16.Toxic.from_seed(BN254))
        self.opk = cpu.ProvingKey.setup(oc, self.tb)
        self.raw = self.opk.serialize()
        self.mats = [oc.csr(k) for k in range(3)]
        self.z = oc.assignment()
        self.dense = np.array(sl.uniform_fr(BN254, oc.m, 0x5EED0191), copy=True)
        self.dense[:32] = self.z[:32]
        # what the case is there for, on the model: the ones bucket of window 0 spans 170 one-entry slices (ten times
        # MSM_HEAVY = 16: a heavy bucket).  (Every variable of this circuit occurs in B — a boolean row names its variable on both
        # sides — so the thinned B list and the lanes that sit bases at infinity out are forced: SHA_KNOBS)
        vals = self.z.reshape(-1, 32)
        self.ones = int(((vals[:, 0] == 1) & (vals[:, 1:] == 0).all(axis=1)).sum())
        assert self.ones >= 10 * 16, self.ones

    @functools.lru_cache(maxsize=None)
    def want(self, which, r, s):
        if which == "bits":
            return cpu.trapdoor(self.oc, self.tb, self.z, r, s)
        return cpu.prove(self.oc, self.opk, self.dense, r, s)[0]


@functools.lru_cache(maxsize=None)
def sha_case():
    return ShaCase()


SHA_KNOBS = {1: {"b_sort": 1, "skip_inf": 1}, 0: {}}       # by heavy_runs: the B family on a sorted list of its own, lanes always sit out; the defaults
SHA_DEFAULTS = {"msm_min_slice": 8, "heavy_runs": 1, "b_sort": 0, "skip_inf": 0}


def sha_run(env, heavy_runs, plan):
    """`plan`: [("bits" | "dense", proofs in the batch)] over ONE key loaded under msm_min_slice 1"""
    sc, ctx = sha_case(), env.ctx
    try:
        ctx.tune("msm_min_slice", 1)
        ctx.tune("heavy_runs", heavy_runs)
        for knob, value in SHA_KNOBS[heavy_runs].items():
            ctx.tune(knob, value)
        cs = native.ConstraintSystem(ctx, 0, sc.oc.n, sc.oc.l, sc.oc.w, sc.mats)
        pk = native.ProvingKey(ctx, 0, sc.raw)
        try:
            for which, n in plan:
                z = sc.z if which == "bits" else sc.dense
                rs = batch_rnds(n)
                if n == 1:
                    proofs = [native.prove_g16(ctx, pk, cs, z, *rs[0])]
                else:
                    proofs, _ = native.prove_g16_batch(ctx, pk, cs, np.concatenate([z] * n), rs)
                for i in range(n):
                    assert proofs[i] == sc.want(which, *rs[i]), (which, "proof %d of %d" % (i, n), "heavy_runs %d" % heavy_runs)
        finally:
            pk.close()
            cs.close()
    finally:
        for knob, value in SHA_DEFAULTS.items():
            ctx.tune(knob, value)


# ------------------------------------------------------------------ once each
def failing_rows(mats, z, r):
    vals = [int.from_bytes(z[32 * i:32 * i + 32].tobytes(), "little") for i in range(z.size // 32)]
    ev = lambda m, k: sum(int.from_bytes(m[2][32 * e:32 * e + 32].tobytes(), "little") * vals[m[1][e]] for e in range(int(m[0][k]), int(m[0][k + 1]))) % r
    return [k for k in range(len(mats[0][0]) - 1) if ev(mats[0], k) * ev(mats[1], k) % r != ev(mats[2], k)]


def checked(env):
    """checked proving refuses an unsatisfying assignment and names its first failing row; the unchecked proof behind it is the oracle's"""
    ctx, cid, L = env.ctx, 0, 3
    pc = sl.proof_case(cid, L, True)
    bad = failing_rows(pc.mats, pc.zbad, sl.CURVES[cid].r)
    assert bad and not failing_rows(pc.mats, pc.zs[0], sl.CURVES[cid].r)
    cs = native.ConstraintSystem(ctx, cid, pc.n, pc.l, pc.oc.w, pc.mats)
    pk = native.ProvingKey(ctx, cid, cpu.ProvingKey.setup(pc.oc, pc.tb).serialize())
    try:
        ctx.set_checked(True)
        try:
            with pytest.raises(native.ZkhipError) as e:
                native.prove_g16(ctx, pk, cs, pc.zbad, 5, 6)
            assert e.value.code == -5 and e.value.unsatisfied == [(0, bad[0], len(bad))], (e.value.code, e.value.unsatisfied, bad)
            assert native.prove_g16(ctx, pk, cs, pc.zs[1], *sl.RS[1]) == pc.g16_want[1], "a satisfying assignment, checked"
        finally:
            ctx.set_checked(False)
        assert native.prove_g16(ctx, pk, cs, pc.zs[0], *sl.RS[0]) == pc.g16_want[0], "the unchecked proof behind the refusal"
    finally:
        pk.close()
        cs.close()


class SharedRig(pq.QRig):
    """test_proof_queue.QRig (its Groth16 half) on a context it does not own"""

    def __init__(self, ctx, n):
        self.lib, self.n, self.curve_id, self.ctx = ctx.lib, n, 0, ctx
        self.case = c = _queue_case(n)
        self.cs = c.system(ctx)
        self.W, self.G = native.ProvingKey(ctx, 0, c.raw), None
        self.za = [native.Assignment(ctx, self.cs, z) for z in c.zs]
        self.zp = [native.pack_assignment(z, ctx.lib) for z in c.zs]
        self.queues = []

    def close(self):
        for d in list(self.queues):
            d.close()
        for h in [self.W] + self.za:
            h.close()
        self.cs.close()


@functools.lru_cache(maxsize=None)
def _queue_case(n):
    return pq.Case(0, n, 0x5EED9000 + 16 * n, gm17=False)


def queue(n):
    def run(env):
        """2 x capacity + 1 tickets from host, resident and packed assignments in turn, then the queue is closed"""
        rig = SharedRig(env.ctx, n)
        try:
            pq.parity_checks(rig, "g16", False)
        finally:
            rig.close()
    return run


def packed(env):
    """upload_packed: the resident assignment made from the packed form proves to the oracle's bytes — a dense assignment and one of
    bits (which does not satisfy the system: the algorithmic oracle)"""
    ctx, cid, L = env.ctx, 0, 5
    pc = sl.proof_case(cid, L, False)
    opk = cpu.ProvingKey.setup(pc.oc, pc.tb)
    rnd = random.Random(0xB175)
    bits = sl.le([1] + [rnd.randrange(2) for _ in range(pc.m - 1)])
    cs = native.ConstraintSystem(ctx, cid, pc.n, pc.l, pc.oc.w, pc.mats)
    pk = native.ProvingKey(ctx, cid, opk.serialize())
    try:
        for z, want in ((pc.zs[0], pc.g16_want[0]), (bits, cpu.prove(pc.oc, opk, bits, *sl.RS[0])[0])):
            a = native.Assignment.from_packed(ctx, cs, native.pack_assignment(z, ctx.lib))
            assert native.prove_g16_resident(ctx, pk, cs, a, *sl.RS[0]) == want
            a.close()
    finally:
        pk.close()
        cs.close()


def witness(env):
    """upload_witness: a witness file of 257 columns (one more than a workgroup) in reversed order — verdict and inputs from oracle.ir,
    and a changed element named by its row"""
    c = wd.Case(env.ctx, 0, *wd.split_ids(257), seed=0xC0 + 257)
    try:
        assert c.upload(wd.witness_file(c.entries()[::-1])) == (NONE, c.inputs())
        k = 255
        changed = dict(c.values)
        changed[c.ids[k]] = (c.values[c.ids[k]] + 1) % c.curve.r
        assert c.upload(wd.witness_file(c.entries(changed))) == ((k, 1), c.inputs(changed))
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def _exec_program():
    r = BN254.r
    params, st = dx.random_program(r, 0x5EED + 200, 200)
    return params, st, dx.draw(random.Random(200), r, 3, 64)


def compute_witness(count):
    def run(env):
        """zkhip_compute_witness of `count` instances over a 200-statement program against tests/exec_ref.py: files, inputs, assignments"""
        params, st, rows = _exec_program()
        b = dx.Built(env.ctx, 0, params, st, return_count=2)
        try:
            b.assert_all_good(rows[:count])
        finally:
            b.close()
    return run


VERIFY_COUNTS = (1, 64, 65)


def verify(scheme):
    def run(env):
        """verify_*_batch at 1, 64 and 65 items (eight items to a workgroup): the prover's proofs are accepted — and they are the
        oracle's bytes — and the last item, whose last input is changed, is not"""
        ctx = env.ctx
        fn = native.verify_g16_batch if scheme == "g16" else native.verify_gm17_batch
        raw, proofs, inputs = dv.make_proofs(ctx, 0, scheme, 5, 3)
        vk = native.VerificationKey(ctx, 0, raw, scheme=scheme)
        try:
            for count in VERIFY_COUNTS:
                ins = [list(inputs[i % 3]) for i in range(count)]
                ins[-1][-1] = (ins[-1][-1] + 1) % BN254.r
                got = list(fn(ctx, vk, [proofs[i % 3] for i in range(count)], dv.inputs_bytes(ins)))
                assert got == [1] * (count - 1) + [0], (scheme, count, got)
        finally:
            vk.close()
    return run


@functools.lru_cache(maxsize=None)
def _pairing_items():
    """test_device_verify's items: e(a P, b Q) e(-(a b + bad) P, Q), bad at every third"""
    G1, G2 = dv.groups_of(BN254)
    rnd = random.Random(77)
    items, want = [], []
    for i in range(max(VERIFY_COUNTS)):
        a, b = rnd.randrange(1, BN254.r), rnd.randrange(1, BN254.r)
        bad = i % 3 == 1
        items.append([(G1.amul(G1.gen, a), G2.amul(G2.gen, b)), (G1.aneg(G1.amul(G1.gen, (a * b + bad) % BN254.r)), G2.gen)])
        want.append(0 if bad else 1)
    return items, want


def pairing_products(env):
    items, want = _pairing_items()
    for count in VERIFY_COUNTS:
        assert dv.run_items(env.ctx, BN254, 0, items[:count]) == want[:count], count


# ------------------------------------------------------------------ the pool of (a)
EMU, GPU = ("emu",), ("gpu",)
POOL = (
    [ntt_step(0, lg) for lg in (0, 1, 5, 10)] + [ntt_step(0, EMU_NTT_MAX, EMU), ntt_step(0, 12, GPU), ntt_step(1, 5), ntt_step(1, 11), ntt_step(2, 5)]
    + [Step("ntt-bn254-2^9-three-pass", "ntt", (9,), (0, "fr"), three_pass)]
    + [forced_msm(cid, group, c) for cid in (0, 1) for group in (1, 2) for c in (4, 9)]
    + [geometry_step(name) for name in geo.CASES]
    + [Step("msm-degenerate-bn254-G1-c8", "msm", (360, DEG_SHAPE["sets"] * DEG_SHAPE["K"]), (0, 1), degenerate)]
    + [g16_step(0, 1), g16_step(0, 3, True), g16_step(0, 5), g16_step(0, 8, True, GPU), g16_step(0, 11, False, GPU), g16_step(1, 1)]
    + [Step("g16-bls12_377-1", "g16", (sl.synth_dims(1)[2], 1), (2, "proof"), lambda env: sl.check_g16_377(env.ctx, 1))]
    + [gm17_step(0, 1), gm17_step(0, 3, True), gm17_step(0, 4), gm17_step(0, 10, False, GPU)]
    + [Step("sha-heavy-runs-%d" % h, "sha", (SHA_N,), (0, "proof"), lambda env, h=h: sha_run(env, h, [("bits", 1)])) for h in (1, 0)]
    + [Step("upload-packed", "packed", (32,), (0, "proof"), packed), Step("upload-witness", "witness", (257,), (0, "fr"), witness)]
    + [Step("compute-witness-%d" % k, "exec", (k,), (0, "fr"), compute_witness(k)) for k in (3, 1)]
    + [Step("checked-unsatisfied", "checked", (8,), (0, "proof"), checked), Step("queue-2cap+1", "queue", (29,), (0, "proof"), queue(29))]
    + [Step("verify-%s-1-64-65" % s, "verify-" + s, (65,), (0, "pairing"), verify(s)) for s in ("g16", "gm17")]
    + [Step("pairing-products-1-64-65", "pairing", (65,), (0, "pairing"), pairing_products)]
)
FAMILIES = sorted({s.family for s in POOL})
BY_NAME = {s.name: s for s in POOL}
assert len(BY_NAME) == len(POOL)


def pool(backend, family=None):
    return [s for s in POOL if backend in s.backends and family in (None, s.family)]


def test_the_pool_reaches_what_it_is_there_for():
    """On the model alone: the transforms' pass structures, both placements of the sort, the scans, the half shapes' real padding."""
    for backend in ("emu", "gpu"):
        logs = [s.size[0] for s in pool(backend, "ntt") if s.first[0] == 0 and "three" not in s.name]
        assert {sl.ntt_plan(lg)["passes"] for lg in logs} == {1, 2} and {0, 1, 5, 10} <= set(logs)
        names = {s.name for s in pool(backend)}
        assert {"msm-geometry-" + n for n in geo.CASES} <= names and len(geo.CASES) == 8
    for L in (3, 8):                                  # D0 < D: the SAP of a half shape leaves a quarter of its domain and more empty
        n, l, m, N = sl.synth_dims(L, True)
        D0 = 2 * n + 2 * (l - 1) + 1
        assert D0 < sl.sap_dims(n, l, m)[1] and 4 * D0 <= 3 * sl.sap_dims(n, l, m)[1]
    assert pq.Case is not None and NSLOTS + 1 == 4


# ------------------------------------------------------------------ (a) filled allocations
def filled(backend, word, family, geom):
    set_fill(backend, word)
    ctx = None
    try:
        ctx = make_context(backend)                   # created under the fill: its slots, sorts, lanes and streams' buffers come filled
        env = Env(backend, ctx, geom)
        for step in sorted(pool(backend, family), key=lambda s: s.size):
            step(env)
    finally:
        try:
            if ctx is not None:
                ctx.close()
        finally:
            set_fill(backend, 0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("word", [SMALL, BYTES], ids=["small", "bytes"])
def test_filled(case, word, family):
    filled("emu", word, family, case)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_gpu_filled(case, family):
    filled("gpu", SMALL, family, case)


def test_the_fill_in_the_emulators_allocator(tmp_path):
    """tests/host/alloc_fill.cpp — a stand-alone program on the CPU, under ASan + UBSan — holds dev_alloc and host_alloc_pinned of
    the ZK_EMU half of csrc/devrt.h to the fill's contract: off by default, every byte of the block while it is on."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "alloc_fill")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_EMU", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(here, "..", "zokrates_amd", "csrc"),
                           os.path.join(here, "host", "alloc_fill.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "61 cases, 0 failures" in out.stderr, out.stderr


def test_the_knob_is_declared_and_not_read_from_the_environment():
    """ZKHIP_TUNE_ALLOC_FILL is id 30, behind exec_chunk, in the header and in the binding; it is not read from the environment"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "zkhip.h")).read()
    assert "#define ZKHIP_TUNE_ALLOC_FILL 30" in header and "TESTS ONLY" in header
    assert native.Context.TUNABLES["alloc_fill"] == 30 == native.Context.TUNABLES["exec_chunk"] + 1
    csrc = os.path.join(root, "zokrates_amd", "csrc")
    for name in os.listdir(csrc):
        if os.path.isfile(os.path.join(csrc, name)):
            assert "ZKHIP_ALLOC_FILL" not in open(os.path.join(csrc, name)).read(), name


# ------------------------------------------------------------------ (b) shrinking and changing shapes in one context
def by_name(name):
    return lambda env: BY_NAME[name](env)


def seq_g2_then_g1(env):
    return [dirty_msm_g2, small_msm_g1]


def seq_msm_widths(env):
    return [by_name("msm-geometry-c17"), by_name("msm-bn254-G1-c4"), by_name("msm-bn254-G2-c4"), by_name("msm-geometry-c14-one-lane"),
            by_name("msm-bn254-G1-c9"), by_name("msm-bn254-G2-c9")]


def seq_schemes(env):
    L = top_L(env.backend)
    return [lambda e: g16_batch(e.ctx, 0, L, bound=True), lambda e: gm17_batch(e.ctx, 0, 3, half=True, bound=False), by_name("g16-bn254-1"),
            lambda e: gm17_batch(e.ctx, 0, 4, bound=True), by_name("gm17-bn254-4"), by_name("g16-bn254-3-half")]


def seq_heavy_then_dense(env):
    """one key: a batch of nslots + 1 witnesses of bits (heavy buckets in every slot), then the dense assignment, whose buckets are
    all light: a heavy list from before must not be believed; and once more without the heavy-run kernel"""
    return [lambda e: sha_run(e, 1, [("bits", NSLOTS + 1), ("dense", 1), ("bits", 1), ("dense", NSLOTS + 1)]),
            lambda e: sha_run(e, 0, [("bits", NSLOTS + 1), ("dense", 1)])]


def seq_queues(env):
    return [queue(400 if env.backend == "emu" else 3000), queue(29)]


def seq_transforms(env):
    two = EMU_NTT_MAX if env.backend == "emu" else 12
    return [by_name("ntt-bn254-2^%d" % two), by_name("ntt-bls12_381-2^11"), by_name("ntt-bn254-2^10"), by_name("ntt-bn254-2^5"), by_name("ntt-bn254-2^1"),
            by_name("ntt-bn254-2^0")]


def seq_checked_then_unchecked(env):
    return [lambda e: g16_batch(e.ctx, 0, top_L(e.backend)), checked]


def seq_compute_witness(env):
    return [compute_witness(64), compute_witness(1)]


DESCENDING = {"msm": ("msm",), "proofs": ("g16", "gm17", "sha", "checked", "queue", "packed"), "fr": ("ntt", "witness", "exec"),
              "pairings": ("verify-g16", "verify-gm17", "pairing")}
assert sorted(f for fs in DESCENDING.values() for f in fs) == FAMILIES


def descending(group):
    def seq(env):
        """three dirtying calls, then the families of the group, each from its largest shape of the pool to its smallest"""
        out = [lambda e: g16_batch(e.ctx, 0, top_L(e.backend), bound=True), dirty_msm_g2, lambda e: gm17_batch(e.ctx, 0, 4)]
        for family in DESCENDING[group]:
            out += sorted(pool(env.backend, family), key=lambda s: s.size, reverse=True)
        return out
    seq.__name__ = "seq_descending_" + group
    return seq


SEQUENCES = {f.__name__[4:]: f for f in (seq_g2_then_g1, seq_msm_widths, seq_schemes, seq_heavy_then_dense, seq_queues, seq_transforms,
                                         seq_checked_then_unchecked, seq_compute_witness) + tuple(descending(g) for g in DESCENDING)}


def run_sequence(backend, name, geom):
    ctx = make_context(backend)
    try:
        env = Env(backend, ctx, geom)
        for k, call in enumerate(SEQUENCES[name](env)):
            try:
                call(env)
            except AssertionError as e:
                raise AssertionError("sequence %s, call %d: %s" % (name, k, e)) from e
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_sequence(case, name):
    run_sequence("emu", name, case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_gpu_sequence(case, name):
    run_sequence("gpu", name, case)


# ------------------------------------------------------------------ the walk
WALK_STEPS, WALK_SEED = 40, 0x0A11C000


def walk_misses(backend, steps):
    """what the model asks of a walk and this one lacks: every family of the pool directly behind a strictly larger call of its own
    family (where the pool holds two such shapes) and directly behind a call that ended on another curve or group"""
    p = pool(backend)
    shrinkable = {a.family for a in p for b in p if larger(a, b)}
    shrunk = {b.family for a, b in zip(steps, steps[1:]) if larger(a, b)}
    moved = {b.family for a, b in zip(steps, steps[1:]) if a.last != b.first}
    return sorted(("shrinks", f) for f in shrinkable - shrunk) + sorted(("moves", f) for f in set(FAMILIES) - moved)


@functools.lru_cache(maxsize=None)
def walk_plan(backend):
    """(seed, steps): a family drawn first, then one of its shapes, so that a family of one shape comes up as often as one of twenty;
    two times in five, where the pool has one, a strictly smaller shape of the family just run"""
    for seed in range(WALK_SEED, WALK_SEED + 2000):
        rnd = random.Random(seed)
        steps = []
        for _ in range(WALK_STEPS):
            smaller = [s for s in pool(backend) if steps and larger(steps[-1], s)]
            if smaller and rnd.random() < 0.4:
                steps.append(rnd.choice(smaller))
            else:
                steps.append(rnd.choice(pool(backend, rnd.choice(FAMILIES))))
        if not walk_misses(backend, steps):
            return seed, steps
    raise AssertionError("no seed gives a walk that meets the model's conditions")


@pytest.mark.parametrize("backend", ["emu", "gpu"])
def test_the_walk_meets_its_conditions(backend):
    """no library: the conditions hold for the walk both halves run, by construction, and the walk is a function of its seed"""
    seed, steps = walk_plan(backend)
    assert len(steps) == WALK_STEPS and walk_misses(backend, steps) == []
    assert {s.family for s in steps} == set(FAMILIES)
    assert len({s.first[0] for s in steps}) == 3 and {"g16", "gm17"} <= {s.family for s in steps}
    assert walk_misses(backend, steps[:1]) != []
    walk_plan.cache_clear()
    assert walk_plan(backend) == (seed, steps)


def run_walk(backend, geom):
    seed, steps = walk_plan(backend)
    ctx = make_context(backend)
    try:
        env = Env(backend, ctx, geom)
        for k, step in enumerate(steps):
            try:
                step(env)
            except AssertionError as e:
                raise AssertionError("walk %#x, step %d (behind %s): %s" % (seed, k, steps[k - 1] if k else None, e)) from e
    finally:
        ctx.close()


def test_walk(case):
    run_walk("emu", case)


@pytest.mark.gpu
def test_gpu_walk(case):
    run_walk("gpu", case)
