"""The size ladder: every domain size from 2^0 to 2^22 against the oracle.  Shared by the emulator and the device halves of
tests/test_size_ladder.py.

The domain size decides which code runs: the pass structure and launch geometry of a transform (get_plan), the window width of a
proof's MSMs (msm_shape over resident tables: a function of the key's size) and of an ad-hoc MSM (msm_shape without a table).  This
module holds

  * the SHAPE MODEL: msm_shape (table mode and ad-hoc mode) and the split and geometry of get_plan, restated in plain Python from
    csrc/msm_geom.h and csrc/ntt_geom.h.  Where the library reports what it chose — the header of a key image (zkhip_pk_export)
    carries c_z, c_h and the transform split — the check functions assert the model against it, and
    tests/test_size_ladder.py::test_the_model_of_the_plan_geometry_against_the_library holds ntt_plan to csrc/ntt_geom.h and
    ::test_the_model_of_the_msm_shape_against_the_library msm_shape to csrc/msm_geom.h, key by key (the ad-hoc width included, which
    the library reports nowhere else);
  * the RUNG LISTS of the transforms, the proofs and the ad-hoc MSM, and what the model says each rung reaches (`coverage`);
  * the CHECK FUNCTIONS, byte-exact against oracle.cpu (BN254, BLS12-381), tests/bls377_ref.py (BLS12-377) or a closed form.  Nothing
    compares the device with itself or with the emulator, and nothing has a tolerance.

The ladder runs on the library's defaults.  The few plans and widths no default reaches (a cols or rows pass shorter than 2^5, three
passes below 2^23, 2-bit windows over a key's tables) are reached on a context of the test's own through zkhip_ctx_tune."""
import functools
import random
import struct

import numpy as np

import bls377_ref as ref
from ntt_structured import DIRS, check_structured
from oracle import cpu, formats
from oracle import gm17 as ogm17
from oracle import groth16 as g16
from oracle.fields import BN254, BLS12_381
from zokrates_amd import native, synth

CURVES = {0: BN254, 1: BLS12_381, 2: ref.CURVE}
BITS = {0: 254, 1: 255, 2: 253}                     # Fr::Params::BITS

# ------------------------------------------------------------------ the shape model: msm_shape
MSM_COARSE_BITS = 8                                 # msm_geom.h: keys per coarse bin = 2^8
MSM_SORT_MAX_KH = 1 << 15                           # counters of one sort workgroup's histogram
MSM_AUTO_MAX_C, MSM_ADHOC_MAX_C = 17, 16


def windows(bits, c):
    return (bits + 1 + c - 1) // c


def adhoc_window(n, bits):
    """The window width an ad-hoc MSM of n points picks by itself (msm_shape without a table): about log2(n) - 5, moved to the
    nearest width whose top window is full or whose top buckets stay below 4096 points each."""
    lg = max(n, 1).bit_length() - 1
    want = max(2, min(MSM_ADHOC_MAX_C, lg - 5))
    for d in range(15):
        for cand in (want + d, want - d):
            if cand < 2 or cand > MSM_ADHOC_MAX_C:
                continue
            W = windows(bits, cand)
            top_bits = bits + 1 - (W - 1) * cand
            if top_bits >= cand or (n >> (top_bits - 1)) <= 4096:
                return cand
    return want


def table_window(m, bits):
    """The window width of a resident key's MSM over m entries (msm_shape with tables): the fewest windows the widest admissible
    width gives, and of the widths with that many windows the narrowest."""
    cmax = max(2, min(MSM_AUTO_MAX_C, max(m, 1).bit_length()))
    wmin = windows(bits, cmax)
    c = cmax
    while c > 2 and windows(bits, c - 1) == wmin:
        c -= 1
    return c


def msm_shape(n, bits, table, force_c=0):
    """What msm_shape and msm_prepare derive from (n, scalar width): the width, the windows, which placement kernel sorts (one level
    below 2^MSM_COARSE_BITS buckets, coarse + fine from there), the histogram halves of a 17-bit window, the fold geometry."""
    c = force_c or (table_window(n, bits) if table else adhoc_window(n, bits))
    K = 1 << (c - 1)
    kh = min(K, MSM_SORT_MAX_KH)
    Lw = min(K, 256)
    return dict(c=c, W=windows(bits, c), K=K, sets=1 if table else windows(bits, c), halves=K // kh,
                two_level=(1 << MSM_COARSE_BITS) <= K <= (1 << 16), Lw=Lw, H=K // Lw)


def key_windows(curve_id, m, N):
    """(c_z, c_h) of a resident key of m variables over a domain of N: the four lanes over z (the fused A / B1 / L launch and the G2
    launch) run over m + 2 entries, the h table over N (finish_tables)."""
    return table_window(m + 2, BITS[curve_id]), table_window(N, BITS[curve_id])


# ------------------------------------------------------------------ the shape model: get_plan
NTT_SINGLE_MAX_LOG, NTT_MAX_SUBLOG, NTT_COLS = 10, 11, 2          # the defaults of zkhip_ctx (core.cuh)


def ntt_plan(logN, single_max=NTT_SINGLE_MAX_LOG, sub=NTT_MAX_SUBLOG, ccols=NTT_COLS):
    """The split and launch geometry of get_plan (csrc/ntt_geom.h: ntt_geom) for a domain of 2^logN."""
    assert 0 <= logN <= 3 * sub
    if logN <= single_max and logN <= sub:
        log1, log2, log3 = 0, logN, 0
    elif logN <= 2 * sub:
        log1 = logN // 2
        log2, log3 = logN - log1, 0
    else:
        log1 = logN // 3
        log2 = (logN - log1) // 2
        log3 = logN - log1 - log2
    N, N1, N2, N3 = 1 << logN, 1 << log1, 1 << log2, 1 << log3
    Nb = N2 * N3
    last = N3 if log3 else N2                                      # length of the rows pass's sequences
    nrows = N // last
    tile_rows = max(last, min(N, 1024))
    R = 1 if log1 == 0 else max(1, min(nrows, tile_rows // last))
    cols_per_wg = lambda ncols, n: max(1, min(ncols, max(ccols, 1024 // max(n, 1))))
    threads = lambda butterflies: min(512, max(64, (butterflies + 63) // 64 * 64))
    smem = lambda nseq, n: 9 * nseq * (n + (n >> 5) + 1) * 4
    C_cols = cols_per_wg(Nb, N1)
    assert Nb % C_cols == 0 and nrows % R == 0
    p = dict(logN=logN, log1=log1, log2=log2, log3=log3, passes=1 + (log1 > 0) + (log3 > 0), split=log1 | (log3 << 8),
             R_rows=R, C_cols=C_cols, threads_cols=threads(C_cols * N1 // 4), threads_rows=threads(R * last // 4),
             smem_cols=smem(C_cols, N1), smem_rows=smem(R, last))
    if log3:
        C_mid = cols_per_wg(N3, N2)
        assert N3 % C_mid == 0 and N1 <= 65535
        p.update(C_mid=C_mid, threads_mid=threads(C_mid * N2 // 4), smem_mid=smem(C_mid, N2))
    assert max(p["smem_cols"], p["smem_rows"], p.get("smem_mid", 0)) <= 160 * 1024          # the LDS of a gfx950 workgroup
    return p


# ------------------------------------------------------------------ the rungs
NTT_LOGS = tuple(range(0, 23))                      # curves 0 and 1: every size against cpu.ntt; structured vectors up to ...
NTT_STRUCTURED_MAX = 14                             # ... 2^14 (their closed forms are Python)
NTT_LOGS_377 = tuple(range(0, 14))                  # curve 2: structured vectors (Python transform up to 2^10, closed forms above)
# plans no default reaches, on a context of the test's own: {name: (knob, value, sizes)}
#   two passes whose cols and rows sub-transforms are shorter than 2^5 (the default first takes two passes at 2^11 = 2^5 x 2^6);
#   three passes below 2^23 (2^9 ... 2^12 as 2^3 x 2^3 x 2^3 ... 2^4 x 2^4 x 2^4)
NTT_TUNED = {"short-two-pass": ("ntt_single_max_log", 1, tuple(range(2, 11))), "three-pass": ("ntt_max_sublog", 4, (9, 10, 11, 12))}

PROOF_LS = tuple(range(1, 20))                      # curves 0 and 1: the domain 2^L of synth.circuit(curve, L)
PROOF_HALF_LS = (3, 8, 9, 15)                       # the second shape: n + l = 2^(L-1) + 1, the domain half empty
PROOF_SETUP_MAX, PROOF_UNSAT_MAX = 12, 14           # key bytes against cpu.ProvingKey.setup; an unsatisfying assignment against cpu.prove
GM17_MAX_DOMAIN_LOG = 19                            # GM17 runs where its SAP domain (2^(L+1) for these circuits) stays at or below this
PROOF_LS_377 = tuple(range(1, 14))                  # curve 2: up to the rung measured in test_size_ladder.py's docstring
PROOF_SETUP_377_MAX = 5                             # ... and its key bytes against the Python setup (a scalar multiplication per query entry)
ADHOC_WIDTHS = tuple(range(2, 17))
ADHOC_G2_MAX_N = 4096


def synth_dims(L, half=False):
    """(n, l, m, N) of a ladder circuit: synth.circuit(curve, L) has n = 2^L - 2 rows, l = 2 and m = n + 4 variables; the second
    shape has n + l = 2^(L-1) + 1, one row more than fits the domain below."""
    n = (1 << (L - 1)) - 1 if half else (1 << L) - 2
    return n, 2, n + 4, 1 << L


def sap_dims(n, l, m):
    """(variables, domain) of the SAP that GM17 makes of an R1CS (oracle.gm17.sap_shape)"""
    M, D0 = 1 + 2 * (l - 1) + (m - l) + n, 2 * n + 2 * (l - 1) + 1
    D = 1
    while D < D0:
        D *= 2
    return M, D


def gm17_runs(L, half=False):
    n, l, m, _ = synth_dims(L, half)
    return sap_dims(n, l, m)[1] <= 1 << GM17_MAX_DOMAIN_LOG


@functools.lru_cache(maxsize=None)
def adhoc_rungs(curve_id):
    """{width: the smallest n at which zkhip_msm picks it by itself}.  adhoc_window is piecewise constant in n: it changes where
    floor(log2 n) does and where n >> (top_bits - 1) passes 4096, so the candidates are those places."""
    bits = BITS[curve_id]
    cands = sorted({1 << k for k in range(0, 23)} | {4097 << s for s in range(0, 11)})
    out = {}
    for n in cands:
        if n <= 1 << 22:
            out.setdefault(adhoc_window(n, bits), n)
    return out


ADHOC_FORCED_N = 1 << 13


def adhoc_cases(curve_id):
    """[(width, n, forced)]: every width the rule picks by itself at its smallest n (width 2 also at its largest, 255: at n = 1 the
    scalars are a single r - 1), and the widths it never picks — their top window would hold a few bits only — under msm_c"""
    auto = adhoc_rungs(curve_id)
    out = [(c, n, False) for c, n in sorted(auto.items())] + [(2, 255, False)]
    return sorted(out + [(c, ADHOC_FORCED_N, True) for c in ADHOC_WIDTHS if c not in auto])


def coverage():
    """What the rungs reach, by the model: the sets tests/test_size_ladder.py::test_the_ladder_covers_every_shape asserts on."""
    cov = {"table": {}, "adhoc": {}, "cols": set(), "rows": set(), "passes": {}, "threads": set()}
    for cid in (0, 1, 2):
        t = cov["table"][cid] = {"h": set(), "z": set()}
        for L in (PROOF_LS_377 if cid == 2 else PROOF_LS):
            dims = [synth_dims(L)] + ([synth_dims(L, True)] if cid < 2 and L in PROOF_HALF_LS else [])
            for half, (n, l, m, N) in enumerate(dims):
                cz, ch = key_windows(cid, m, N)
                t["z"].add(cz); t["h"].add(ch)
                if cid < 2 and gm17_runs(L, bool(half)):
                    M, D = sap_dims(n, l, m)
                    cz, ch = key_windows(cid, M, D)
                    t["z"].add(cz); t["h"].add(ch)
        cov["adhoc"][cid] = {c: forced for c, n, forced in adhoc_cases(cid)}
    plans = [ntt_plan(lg) for lg in NTT_LOGS]
    for knob, value, sizes in NTT_TUNED.values():
        plans += [ntt_plan(lg, **{"ntt_single_max_log": dict(single_max=value), "ntt_max_sublog": dict(sub=value)}[knob]) for lg in sizes]
    for p in plans:
        cov["passes"].setdefault(p["passes"], set()).add(p["logN"])
        cov["threads"] |= {p["threads_rows"]} | ({p["threads_cols"]} if p["log1"] else set())
        if p["passes"] == 2:
            cov["cols"].add(p["log1"]); cov["rows"].add(p["log2"])
    return cov


# ------------------------------------------------------------------ helpers
def le(vals, nb=32):
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "little") for v in vals), dtype=np.uint8)


def uniform_fr(curve, n, seed):
    """n values uniform over [0, r) as uint8[n * 32]: rejection from 2^bits on the top limb, nothing masked below the modulus (a draw
    whose top 64 bits equal r's is dropped too: one in 2^60), with r - 1 at 0, n / 2 and n - 1 and 0 at n / 4."""
    r, bits = curve.r, curve.r.bit_length()
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    mask, rtop = np.uint64((1 << (bits - 192)) - 1), np.uint64(r >> 192)
    out[:, 3] &= mask
    todo = np.nonzero(out[:, 3] >= rtop)[0]
    while todo.size:
        out[todo] = rng.integers(0, 1 << 64, size=(todo.size, 4), dtype=np.uint64)
        out[todo, 3] &= mask
        todo = todo[out[todo, 3] >= rtop]
    out = out.view(np.uint8).reshape(n, 32)
    top = np.frombuffer((r - 1).to_bytes(32, "little"), dtype=np.uint8)
    for k in {0, n // 2, n - 1}:
        out[k] = top
    if n > 3:
        out[n // 4] = 0
    return out.reshape(-1)


def image_header(pk):
    """(logN, c_z, c_h, sets, transform split) as the library chose them for this key: PkImageHeader of zkhip_pk_export."""
    img = pk.export_image()
    assert img[:7].tobytes() == b"ZKHIPPK"
    logN, c_z, c_h, sets = struct.unpack_from("<4i", img, 56)
    (split,) = struct.unpack_from("<i", img, 80)
    return logN, c_z, c_h, sets, split


def assert_key_shape(pk, curve_id, m, N, force_c=0, plan={}):
    """the model against what the library chose for this key; `force_c`, `plan`: the knobs the context runs under, if any"""
    logN, c_z, c_h, sets, split = image_header(pk)
    cz, ch = (force_c, force_c) if force_c else key_windows(curve_id, m, N)
    assert (1 << logN, c_z, c_h) == (N, cz, ch), ("the model of msm_shape against the key's header", (logN, c_z, c_h), (N, cz, ch))
    assert sets == 1 | (1 << 8), sets                 # every window multiple resident at these sizes: one bucket set
    assert split == ntt_plan(logN, **plan)["split"], ("the model of get_plan against the key's header", split, ntt_plan(logN, **plan))


# ------------------------------------------------------------------ (b) transforms
_ntt_ref = {}


def ntt_reference(curve_id, logn):
    """(input, {direction: the oracle's bytes}), made once per curve and size"""
    key = (curve_id, logn)
    if key not in _ntt_ref:
        if len(_ntt_ref) >= 2 and logn >= 18:
            _ntt_ref.clear()                          # (five vectors of 2^22 are 640 MiB: the large rungs do not pile up)
        a = uniform_fr(CURVES[curve_id], 1 << logn, 0x51DE0000 + 64 * curve_id + logn)
        _ntt_ref[key] = a, {d: cpu.ntt(curve_id, a, d).tobytes() for d in DIRS}
    return _ntt_ref[key]


def check_ntt(ctx, curve_id, logn):
    """zkhip_ntt in all four directions against cpu.ntt, and the coset round trip"""
    a, want = ntt_reference(curve_id, logn)
    r = CURVES[curve_id].r
    assert a.size == 32 << logn and int.from_bytes(a[:32].tobytes(), "little") == r - 1 == int.from_bytes(a[-32:].tobytes(), "little")
    for d in DIRS:
        assert ctx.ntt(curve_id, a, d).tobytes() == want[d], (CURVES[curve_id].name, logn, d)
    # the coset round trip gives back the input (its first leg is the bytes just held to the oracle)
    assert ctx.ntt(curve_id, np.frombuffer(want["coset_fft"], dtype=np.uint8), "coset_ifft").tobytes() == a.tobytes(), ("round trip", logn)


def check_ntt_rung(ctx, curve_id, logn):
    if curve_id < 2:
        check_ntt(ctx, curve_id, logn)
        if logn <= NTT_STRUCTURED_MAX:
            check_structured(ctx, CURVES[curve_id], logn)
    else:
        check_structured(ctx, CURVES[curve_id], logn)


def check_ntt_tuned(make_ctx, curve_id, name):
    """the plans of NTT_TUNED on a context of the test's own (the plan cache is per context; the context is closed, not restored)"""
    knob, value, sizes = NTT_TUNED[name]
    c2 = make_ctx()
    try:
        c2.tune(knob, value)
        for logn in sizes:
            check_ntt(c2, curve_id, logn)
    finally:
        c2.close()


# ------------------------------------------------------------------ (c) witness map and proofs, curves 0 and 1
RS = ((0x1234567890abcdef, 0xfedcba9876543210fedcba), (3, 4), (0, 9))
SEEDS = (0x5EED0001, 0x5EED0002)


class ProofCase:
    """A ladder circuit, two satisfying assignments and every expected byte string, from the oracle alone (made once per rung and
    shared by the checks of both schemes; the last two rungs are kept)."""

    def __init__(self, curve_id, L, half):
        self.curve_id, self.L, self.half = curve_id, L, half
        curve = CURVES[curve_id]
        n, l, m, N = synth_dims(L, half)
        if half:
            oc = cpu.Circuit.synth(curve_id, n, 0x5EED1000 + L)
            self.mats = [oc.csr(k) for k in range(3)]
            z = oc.assignment()
            # the second assignment: the chain again from other free variables (row k of the dense chain defines variable 4 + k)
            self.zs = [z, le(self._chain_again(oc, curve.r, z))]
        else:
            circ = synth.circuit(curve_id, L, seed=0x1ADD00 + L)
            self.mats = circ.mats()
            oc = cpu.Circuit.from_csr(curve_id, circ.n, circ.l, circ.w, self.mats)
            self.zs = [circ.assignment(s + L) for s in SEEDS]
        assert (oc.n, oc.l, oc.m, oc.N) == (n, l, m, N), ((oc.n, oc.l, oc.m, oc.N), (n, l, m, N))
        self.oc, self.n, self.l, self.m, self.N = oc, n, l, m, N
        self.tox = synth.toxic_waste(curve_id, 0xBEEF + L)
        self.tb = b"".join(int(v).to_bytes(32, "little") for v in self.tox)
        self.zbad = np.array(self.zs[0], copy=True)
        self.zbad[32 * (l + 1)] ^= 1                   # (a free variable of the chain: the rows after it no longer hold)

    def _chain_again(self, oc, r, z):
        rnd = random.Random(self.L)
        vals = [int.from_bytes(z[32 * i:32 * i + 32].tobytes(), "little") for i in range(oc.m)]
        vals[1:4] = [rnd.randrange(r) for _ in range(3)]
        (rpa, ca, va), (rpb, cb, vb), (rpc, cc, vc) = self.mats
        ev = lambda rp, col, val, k: sum(int.from_bytes(val[32 * e:32 * e + 32].tobytes(), "little") * vals[col[e]] for e in range(int(rp[k]), int(rp[k + 1]))) % r
        for k in range(oc.n):
            assert rpc[k + 1] - rpc[k] == 1 and int.from_bytes(vc[32 * int(rpc[k]):32 * int(rpc[k]) + 32].tobytes(), "little") == 1
            vals[cc[int(rpc[k])]] = ev(rpa, ca, va, k) * ev(rpb, cb, vb, k) % r
        return vals

    @functools.cached_property
    def wmaps(self):
        return [cpu.witness_map(self.oc, z).tobytes() for z in self.zs]

    @functools.cached_property
    def g16_want(self):
        """the closed forms of the batch: (assignment 0, RS[0]), (assignment 1, RS[1]), (assignment 0, RS[2])"""
        return [cpu.trapdoor(self.oc, self.tb, self.zs[i % 2], *RS[i]) for i in range(3)]

    @functools.cached_property
    def tb17(self):
        return b"".join(int(self.tox[i]).to_bytes(32, "little") for i in (0, 1, 2, 4))

    @functools.cached_property
    def gm17_want(self):
        return [cpu.gm17_trapdoor(self.oc, self.tb17, self.zs[i % 2], RS[i][0], RS[i][1]) for i in range(3)]


@functools.lru_cache(maxsize=2)
def proof_case(curve_id, L, half=False):
    return ProofCase(curve_id, L, half)


def check_g16(ctx, curve_id, L, half=False, force_c=0, plan={}):
    """One rung of Groth16 on `ctx`: the key (made on the device for a full domain, by the oracle for a half-empty one), the witness
    map, lone proofs over the key as loaded and bound, a resident batch of three over two assignments, an unsatisfying assignment."""
    case = proof_case(curve_id, L, half)
    oc = case.oc
    cs = native.ConstraintSystem(ctx, curve_id, case.n, case.l, oc.w, case.mats)
    opk = None
    if half:
        opk = cpu.ProvingKey.setup(oc, case.tb)
        raw = opk.serialize()
    else:
        raw = native.setup_g16(ctx, cs, case.tox)
        if L <= PROOF_SETUP_MAX:
            opk = cpu.ProvingKey.setup(oc, case.tb)
            assert raw.tobytes() == opk.serialize().tobytes(), "device setup differs from the oracle's key"
    for z, want in zip(case.zs, case.wmaps):
        assert cs.witness_map(z).tobytes() == want, "witness map"
    pk = native.ProvingKey(ctx, curve_id, raw)
    try:
        assert_key_shape(pk, curve_id, case.m, case.N, force_c, plan)
        want = case.g16_want
        assert native.prove_g16(ctx, pk, cs, case.zs[0], *RS[0]) == want[0], "lone proof, key as loaded"
        zas = [native.Assignment(ctx, cs, z) for z in case.zs]
        proofs, _ = native.prove_g16_resident_batch(ctx, pk, cs, [zas[0], zas[1], zas[0]], list(RS))
        assert proofs == want, "resident batch of three over two assignments"
        if L <= PROOF_UNSAT_MAX:
            opk = opk or cpu.ProvingKey.parse(curve_id, raw.tobytes())
            assert native.prove_g16(ctx, pk, cs, case.zbad, 5, 6) == cpu.prove(oc, opk, case.zbad, 5, 6)[0], "unsatisfying assignment"
        pk.bind(cs)
        assert pk.is_bound(cs)
        assert native.prove_g16(ctx, pk, cs, case.zs[0], *RS[0]) == want[0], "lone proof, key bound"
        assert native.prove_g16(ctx, pk, cs, case.zs[1], *RS[1]) == want[1], "lone proof of the other assignment, key bound"
        for za in zas:
            za.close()
    finally:
        pk.close()
        cs.close()


def check_gm17(ctx, curve_id, L, half=False):
    """The same rung under GM17: its SAP has 2^(L+1) + 1 variables over a domain of 2^(L+1), one rung above Groth16's."""
    assert gm17_runs(L, half)
    case = proof_case(curve_id, L, half)
    oc = case.oc
    t4 = tuple(case.tox[i] for i in (0, 1, 2, 4))
    cs = native.ConstraintSystem(ctx, curve_id, case.n, case.l, oc.w, case.mats)
    if half:
        raw = cpu.Gm17ProvingKey.setup(oc, case.tb17).serialize()
    else:
        raw = native.setup_gm17(ctx, cs, t4)
        if L <= PROOF_SETUP_MAX:
            assert raw.tobytes() == cpu.Gm17ProvingKey.setup(oc, case.tb17).serialize().tobytes(), "device GM17 setup differs from the oracle's key"
    pk = native.ProvingKey(ctx, curve_id, raw, scheme="gm17")
    try:
        M, D = sap_dims(case.n, case.l, case.m)
        assert_key_shape(pk, curve_id, M, D)
        want = case.gm17_want
        rnds = [(RS[i][0], 7 + i, RS[i][1]) for i in range(3)]          # (d1, d2, r): d2 cancels in the proof
        assert native.prove_gm17(ctx, pk, cs, case.zs[0], *rnds[0]) == want[0], "lone GM17 proof, key as loaded"
        zas = [native.Assignment(ctx, cs, z) for z in case.zs]
        proofs, _ = native.prove_gm17_resident_batch(ctx, pk, cs, [zas[0], zas[1], zas[0]], rnds)
        assert proofs == want, "resident GM17 batch of three over two assignments"
        pk.bind(cs)
        assert pk.is_bound(cs)
        assert native.prove_gm17(ctx, pk, cs, case.zs[0], *rnds[0]) == want[0], "lone GM17 proof, key bound"
        assert native.prove_gm17(ctx, pk, cs, case.zs[1], *rnds[1]) == want[1], "lone GM17 proof of the other assignment, key bound"
        for za in zas:
            za.close()
    finally:
        pk.close()
        cs.close()


# ------------------------------------------------------------------ (c) curve 2: tests/bls377_ref.py
@functools.lru_cache(maxsize=2)
def proof_case_377(L):
    C = ref.CURVE
    n, l, m, N = synth_dims(L)
    cs, z = g16.synthetic_chain(C, n, 0x377000 + L)
    assert (cs.n, cs.l, cs.m, cs.domain_size()) == (n, l, m, N) and cs.is_satisfied(z, C.r)
    rnd = random.Random(0x377 + L)
    z2 = [1] + [rnd.randrange(C.r) for _ in range(3)]
    ev = lambda row: sum(c * z2[j] for j, c in row) % C.r
    for a, b, c in zip(cs.A, cs.B, cs.C):
        assert c == [(len(z2), 1)]
        z2.append(ev(a) * ev(b) % C.r)
    assert cs.is_satisfied(z2, C.r) and z2 != z
    return cs, ref.csr(cs), [z, z2]


def check_g16_377(ctx, L, gm17=False):
    """One rung over BLS12-377, Groth16 or GM17: the same assertions against the Python reference (no algorithmic prover: it is the
    closed form that stays affordable)."""
    C, CID = ref.CURVE, 2
    cs, mats, zs = proof_case_377(L)
    ncs = native.ConstraintSystem(ctx, CID, cs.n, cs.l, cs.w, mats)
    zb = [le(z) for z in zs]
    if gm17:
        tox = ogm17.Toxic.from_seed(C, 0xC0FFEE + L)
        raw = native.setup_gm17(ctx, ncs, (tox.alpha, tox.beta, tox.gamma, tox.t))
        rnds = [(RS[i][0], 7 + i, RS[i][1]) for i in range(3)]
        want = [formats.proof_raw(C, ref.gm17_trapdoor(cs, tox, zs[i % 2], rnds[i][0], rnds[i][2])) for i in range(3)]
        pk = native.ProvingKey(ctx, CID, raw, scheme="gm17")
        dims = sap_dims(cs.n, cs.l, cs.m)
        lone = lambda z, i: native.prove_gm17(ctx, pk, ncs, z, *rnds[i])
        batch = lambda zas: native.prove_gm17_resident_batch(ctx, pk, ncs, zas, rnds)[0]
    else:
        tox = g16.Toxic.from_seed(C, 0xC0FFEE + L)
        raw = native.setup_g16(ctx, ncs, (tox.alpha, tox.beta, tox.gamma, tox.delta, tox.tau))
        want = [formats.proof_raw(C, ref.g16_trapdoor(cs, tox, zs[i % 2], *RS[i])) for i in range(3)]
        pk = native.ProvingKey(ctx, CID, raw)
        dims = (cs.m, cs.domain_size())
        lone = lambda z, i: native.prove_g16(ctx, pk, ncs, z, *RS[i])
        batch = lambda zas: native.prove_g16_resident_batch(ctx, pk, ncs, zas, list(RS))[0]
        for z, b in zip(zs, zb):
            assert ncs.witness_map(b).tobytes() == le(g16.witness_map(C, cs, z)).tobytes(), "witness map"
    try:
        if L <= PROOF_SETUP_377_MAX:
            with ref.oracle_groups():
                okey = ogm17.pk_serialize(C, ogm17.setup(C, cs, tox)[0]) if gm17 else formats.ark_pk_serialize(C, g16.setup(C, cs, tox)[0])
            assert raw.tobytes() == bytes(okey), "device setup differs from the reference's key"
        assert_key_shape(pk, CID, *dims)
        assert lone(zb[0], 0) == want[0], "lone proof, key as loaded"
        zas = [native.Assignment(ctx, ncs, b) for b in zb]
        assert batch([zas[0], zas[1], zas[0]]) == want, "resident batch of three over two assignments"
        pk.bind(ncs)
        assert pk.is_bound(ncs)
        assert lone(zb[0], 0) == want[0] and lone(zb[1], 1) == want[1], "lone proofs, key bound"
        for za in zas:
            za.close()
    finally:
        pk.close()
        ncs.close()


# ------------------------------------------------------------------ (d) ad-hoc MSM at every width
ADHOC_BASE_POOL = 1 << 14        # distinct bases of a rung (test_gpu_parity._bases costs a setup); a larger rung repeats them in turn, under
                                 # other scalars


@functools.lru_cache(maxsize=None)
def _base_pool(curve_id):
    from test_gpu_parity import _bases
    m, g1, g2 = _bases(CURVES[curve_id], ADHOC_BASE_POOL - 4, 100 + ADHOC_BASE_POOL)
    assert m == ADHOC_BASE_POOL
    pb = 2 * CURVES[curve_id].fq_bytes
    return np.array(g1).reshape(m, pb), np.array(g2).reshape(m, 2 * pb)[:ADHOC_G2_MAX_N]


@functools.lru_cache(maxsize=2)
def adhoc_case(curve_id, c, n):
    """(G1 bases, G2 bases or None, scalars, cpu.msm's answers) of the rung (c, n): full-width scalars with 0, 1 and r - 1 among them"""
    curve = CURVES[curve_id]
    p1, p2 = _base_pool(curve_id)
    g1 = np.resize(p1, (n, p1.shape[1])).reshape(-1)
    ks = uniform_fr(curve, n, 0xAD0C + 32 * curve_id + c).reshape(-1, 32)          # r - 1 at 0, n / 2, n - 1 and 0 at n / 4
    if n >= 8:
        ks[n // 4 + 1] = 0
        ks[n // 4 + 1, 0] = 1
    ks = ks.reshape(-1)
    g2 = p2[:n].reshape(-1) if n <= ADHOC_G2_MAX_N else None
    return g1, g2, ks, cpu.msm(curve_id, 1, g1, ks), None if g2 is None else cpu.msm(curve_id, 2, g2, ks)


def check_adhoc_msm(ctx, curve_id, c, n, forced=False):
    """zkhip_msm over n ad-hoc points against cpu.msm: at a width the rule picks by itself for this n, or (`forced`: the widths no n
    picks) under msm_c on `ctx`, which is then a context of the test's own"""
    g1, g2, ks, want1, want2 = adhoc_case(curve_id, c, n)
    assert forced or msm_shape(n, BITS[curve_id], False)["c"] == c
    assert not forced or c not in adhoc_rungs(curve_id)
    if forced:
        ctx.tune("msm_c", c)
    try:
        assert ctx.msm(curve_id, 1, g1, ks) == want1, (CURVES[curve_id].name, c, n)
        if g2 is not None:
            assert ctx.msm(curve_id, 2, g2, ks) == want2, (CURVES[curve_id].name, c, n, "G2")
    finally:
        if forced:
            ctx.tune("msm_c", 0)
