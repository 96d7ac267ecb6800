"""GM17 (BASELINE.json config 5): oracle self-consistency (`-m "not gpu"`), the device path on the TEST-ONLY emulator,
and — `-m gpu` — bit-exact parity of the HIP path through the C ABI.

Reference: /root/reference/zokrates_ark/src/gm17.rs:19-78 (setup / generate_proof), verification equations
/root/reference/zokrates_proof_systems/src/scheme/gm17.rs:168-184."""
import os
import random

import numpy as np
import pytest

from oracle import formats, gm17
from oracle import groth16 as g16
from oracle.curves import groups
from oracle.fields import BN254, BLS12_381
from zokrates_amd import native

CURVES = [BN254, BLS12_381]


def le(vals, nb=32):
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "little") for v in vals), dtype=np.uint8)


def csr_of(rows):
    rp, col, val = [0], [], []
    for row in rows:
        for j, v in row:
            col.append(j)
            val.append(v)
        rp.append(len(col))
    return np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), le(val) if val else np.zeros(0, dtype=np.uint8)


def circuit(curve, n, seed, kind="dense", extra_public=0):
    """Synthetic chain; `extra_public` moves that many leading witness wires into the instance (l > 2) so that the
    f_i rows of the SAP are exercised."""
    cs, z = g16.synthetic_chain(curve, n, seed, kind)
    if extra_public:
        cs.l += extra_public
        cs.w -= extra_public
    return cs, z


def proof_bytes(curve, proof):
    return formats.proof_raw(curve, proof)


# ------------------------------------------------------------------ oracle (CPU)
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_oracle_consistency(curve):
    """O2 (ark's algorithm) == O1 (closed form), O3 accepts, a mutated proof is rejected, the proof depends on
    (d1, d2, r) only through r + d1."""
    cs, z = circuit(curve, 6, 21, extra_public=2)
    assert cs.is_satisfied(z, curve.r)
    M, D0, D = gm17.sap_shape(cs)
    assert (M, D0, D) == (1 + 2 * 3 + cs.w + cs.n, 2 * 6 + 2 * 3 + 1, 32)
    tox = gm17.Toxic.from_seed(curve)
    pk, vk = gm17.setup(curve, cs, tox)
    assert len(pk["a_query"]) == len(pk["b_query"]) == len(pk["c_query_2"]) == M
    assert len(pk["c_query_1"]) == M - cs.l and len(pk["g_gamma2_z_t"]) == D + 1 and len(vk["query"]) == cs.l
    rnd = random.Random(3)
    d1, d2, r_ = (rnd.randrange(curve.r) for _ in range(3))
    ext, h = gm17.witness_map(curve, cs, z, d1, d2)
    assert len(ext) == M and len(h) == D + 1
    proof = gm17.prove(curve, cs, pk, z, d1, d2, r_)
    assert proof == gm17.trapdoor_prove(curve, cs, tox, z, d1, r_)
    assert proof == gm17.prove(curve, cs, pk, z, (d1 + 9) % curve.r, 1, (r_ - 9) % curve.r)
    assert gm17.verify(curve, vk, proof, z[1:cs.l])
    G1, _ = groups(curve)
    assert not gm17.verify(curve, vk, (proof[0], proof[1], G1.aadd(proof[2], G1.gen)), z[1:cs.l])
    assert not gm17.verify(curve, vk, proof, [(z[1] + 1) % curve.r] + z[2:cs.l])


def test_oracle_unsatisfied_assignment_fails_verification():
    curve = BN254
    cs, z = circuit(curve, 5, 22)
    tox = gm17.Toxic.from_seed(curve)
    pk, vk = gm17.setup(curve, cs, tox)
    z = list(z)
    z[-1] = (z[-1] + 1) % curve.r
    assert not gm17.verify(curve, vk, gm17.prove(curve, cs, pk, z, 1, 2, 3), z[1:cs.l])


# ------------------------------------------------------------------ device path (shared by emulator and GPU tests)
def run_device_checks(ctx, curve, n, seed, kind="dense", extra_public=0, verify=True, light=False):
    """Expected values come from the C++ restatement (oracle/c/gm17.hpp), which test_cpp_oracle_matches_python pins
    bit-for-bit on the python one; the pairing check of the device proof uses the python verifier."""
    from oracle import cpu
    cs, z = circuit(curve, n, seed, kind, extra_public)
    tox = gm17.Toxic.from_seed(curve)
    mats = [csr_of(cs.A), csr_of(cs.B), csr_of(cs.C)]
    dcs = native.ConstraintSystem(ctx, curve.curve_id, cs.n, cs.l, cs.w, mats)
    raw = native.setup_gm17(ctx, dcs, (tox.alpha, tox.beta, tox.gamma, tox.t))
    oc = cpu.Circuit.from_csr(curve.curve_id, cs.n, cs.l, cs.w, mats)
    tb = cpu.gm17_toxic_bytes(tox)
    opk = cpu.Gm17ProvingKey.setup(oc, tb)
    assert raw.tobytes() == opk.serialize().tobytes()                         # setup: bit-identical key bytes
    pk = native.ProvingKey(ctx, curve.curve_id, raw, scheme="gm17")
    M, _, D = gm17.sap_shape(cs)
    assert (pk.m, pk.hlen, pk.w, pk.l) == (M, D + 1, M - cs.l, cs.l)
    zb = le(z)
    rnd = random.Random(seed)
    d1, d2, r_ = (rnd.randrange(curve.r) for _ in range(3))
    want = cpu.gm17_trapdoor(oc, tb, zb, d1, r_)
    got, tm = native.prove_gm17(ctx, pk, dcs, zb, d1, d2, r_, want_timings=True)
    assert got == want
    assert got == cpu.gm17_prove(oc, opk, zb, d1, d2, r_)[0]                  # == ark's algorithm, term by term
    if verify:
        assert gm17.verify(curve, gm17.vk_from_pk_bytes(curve, raw), formats.proof_from_raw(curve, got), z[1:cs.l])
    if light:           # the emulator spends ~1 s per proof: the variations below run once per curve there, always on the GPU
        return cs, z, dcs, pk, raw
    # corner cases of the blinding: all zero; r + d1 == 0
    assert native.prove_gm17(ctx, pk, dcs, zb, 0, 0, 0) == cpu.gm17_trapdoor(oc, tb, zb, 0, 0)
    assert native.prove_gm17(ctx, pk, dcs, zb, 5, 7, curve.r - 5) == cpu.gm17_trapdoor(oc, tb, zb, 0, 0)
    # resident assignment, batch with two proofs in flight
    za = native.Assignment(ctx, dcs, zb)
    assert native.prove_gm17(ctx, pk, dcs, za, d1, d2, r_) == want
    proofs, _ = native.prove_gm17_resident_batch(ctx, pk, dcs, [za] * 3, [(d1, d2, r_), (1, 2, 3), (d1, 0, r_)])
    assert proofs[0] == want and proofs[2] == want
    assert proofs[1] == cpu.gm17_trapdoor(oc, tb, zb, 1, 3)
    za.close()
    return cs, z, dcs, pk, raw


_long_batch = {}


def long_batch_case():
    """The circuit, key bytes, seven blinding triples (one with r + d1 == 0) and the closed-form proofs of run_long_batch_checks:
    computed once, shared by the emulator and the GPU test, read only."""
    if not _long_batch:
        from oracle import cpu
        curve = BN254
        cs, z = circuit(curve, 7, 71, extra_public=1)
        mats = [csr_of(cs.A), csr_of(cs.B), csr_of(cs.C)]
        oc = cpu.Circuit.from_csr(curve.curve_id, cs.n, cs.l, cs.w, mats)
        tb = cpu.gm17_toxic_bytes(gm17.Toxic.from_seed(curve))
        raw = cpu.Gm17ProvingKey.setup(oc, tb).serialize()
        rnd = random.Random(71)
        rnds = [tuple(rnd.randrange(curve.r) for _ in range(3)) for _ in range(7)]
        rnds[5] = (rnds[5][0], rnds[5][1], curve.r - rnds[5][0])
        assert len(set(rnds)) == 7 and len({(d1 + r_) % curve.r for d1, _, r_ in rnds}) == 7
        want = [cpu.gm17_trapdoor(oc, tb, le(z), d1, r_) for d1, _, r_ in rnds]
        zbad = list(z)
        zbad[-1] = (zbad[-1] + 1) % curve.r                      # the last wire: only the last row's C mentions it
        dot = lambda row, v: sum(c * v[j] for j, c in row)
        bad = [i for i in range(cs.n) if (dot(cs.A[i], zbad) * dot(cs.B[i], zbad) - dot(cs.C[i], zbad)) % curve.r]
        assert bad == [cs.n - 1] and cs.is_satisfied(z, curve.r)
        _long_batch.update(cs=cs, mats=mats, raw=raw, rnds=rnds, want=want, zb=le(z), zbad=le(zbad), bad_row=bad[0])
    return _long_batch


def run_long_batch_checks(ctx):
    """A resident batch of 2 * nslots + 1 = 7 proofs: every slot is used again within one call, twice.  Each proof against the closed
    form; over the key as loaded and over the bound key; three proofs in flight and one.  Then checked mode: proof 4 of the 7 with one
    broken row is named, alone, the other six are written, and the unchecked batch right behind it succeeds."""
    case = long_batch_case()
    cs, rnds, want = case["cs"], case["rnds"], case["want"]
    dcs = native.ConstraintSystem(ctx, 0, cs.n, cs.l, cs.w, case["mats"])
    pk = native.ProvingKey(ctx, 0, case["raw"], scheme="gm17")
    za, zbad = native.Assignment(ctx, dcs, case["zb"]), native.Assignment(ctx, dcs, case["zbad"])
    try:
        for bound in (False, True):
            if bound:
                pk.bind(dcs)
                assert pk.is_bound(dcs)
            for slots in (3, 1):
                ctx.tune("slots", slots)
                assert native.prove_gm17_resident_batch(ctx, pk, dcs, [za] * 7, rnds)[0] == want, (bound, slots)
            ctx.tune("slots", 3)
            assert ctx.set_checked(True) is False
            with pytest.raises(native.ZkhipError) as e:
                native.prove_gm17_resident_batch(ctx, pk, dcs, [za] * 4 + [zbad] + [za] * 2, rnds)
            assert e.value.code == -5 and e.value.unsatisfied == ctx.unsatisfied() == [(4, case["bad_row"], 1)], bound
            assert "proof 4 of 7: constraint %d of %d is not satisfied (1 in all)" % (case["bad_row"], cs.n) in str(e.value)
            assert e.value.proofs[:4] + e.value.proofs[5:] == want[:4] + want[5:] and e.value.proofs[4] == bytes(len(want[4])), bound
            assert ctx.set_checked(False) is True
            assert native.prove_gm17_resident_batch(ctx, pk, dcs, [za] * 7, rnds)[0] == want, bound
            assert ctx.unsatisfied() == []
    finally:
        ctx.set_checked(False)
        ctx.tune("slots", 3)
        for h in (za, zbad, pk, dcs):
            h.close()


def run_error_checks(ctx):
    curve = BN254
    cs, z, dcs, pk, raw = run_device_checks(ctx, curve, 5, 31, verify=False, light=True)
    with pytest.raises(native.ZkhipError) as e:
        native.ProvingKey(ctx, 0, raw[:-1], scheme="gm17")
    assert e.value.code == -2
    with pytest.raises(native.ZkhipError) as e:                              # a GM17 key is not a Groth16 key
        native.prove_g16(ctx, pk, dcs, le(z), 1, 2)
    assert e.value.code == -1
    with pytest.raises(native.ZkhipError) as e:                              # non-canonical blinding scalar
        native.prove_gm17(ctx, pk, dcs, le(z), curve.r, 0, 1)
    assert e.value.code == -1
    zz = le(z).copy()
    zz[0] = 2
    with pytest.raises(native.ZkhipError) as e:
        native.prove_gm17(ctx, pk, dcs, zz, 1, 2, 3)
    assert e.value.code == -1
    cs2, z2 = circuit(curve, 9, 32)                                           # key / circuit mismatch
    dcs2 = native.ConstraintSystem(ctx, 0, cs2.n, cs2.l, cs2.w, [csr_of(cs2.A), csr_of(cs2.B), csr_of(cs2.C)])
    with pytest.raises(native.ZkhipError) as e:
        native.prove_gm17(ctx, pk, dcs2, le(z2), 1, 2, 3)
    assert e.value.code == -1
    assert native.prove_gm17(ctx, pk, dcs, le(z), 1, 2, 3)                   # the context stays usable


# ------------------------------------------------------------------ emulator (CPU)
@pytest.fixture(scope="module")
def emu_ctx():
    from emu_util import emu_library
    c = native.Context(0, emu_library())
    yield c
    c.close()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_emu_gm17(emu_ctx, curve):
    run_device_checks(emu_ctx, curve, 7, 41, extra_public=1)


def test_emu_gm17_boolean_wires(emu_ctx):
    run_device_checks(emu_ctx, BN254, 20, 42, kind="sha", light=True)


def test_emu_gm17_two_pass_ntt():
    """Force the two-pass NTT (sigma order, permuted g_gamma2_z_t) inside the GM17 prover."""
    from emu_util import emu_library
    os.environ["ZKHIP_NTT_SINGLE_MAX_LOG"] = "2"
    c2 = native.Context(0, emu_library())
    try:
        run_device_checks(c2, BN254, 13, 43, light=True)          # D = 32 -> N1 = 4, N2 = 8
    finally:
        os.environ.pop("ZKHIP_NTT_SINGLE_MAX_LOG")
        c2.close()


def test_emu_gm17_errors(emu_ctx):
    run_error_checks(emu_ctx)


def test_emu_gm17_batch_longer_than_the_slots(emu_ctx):
    run_long_batch_checks(emu_ctx)


def test_slot_sums_layout_host(tmp_path):
    """tests/host/slot_sums_layout.cpp under ASan + UBSan: the layout of a slot's window sums (SlotSums, shared by both provers),
    every accessor written through to the last byte of buffers of exactly the stated sizes.  A stand-alone program on the CPU."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "slot_sums_layout")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_EMU", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(here, "..", "zokrates_amd", "csrc"), os.path.join(here, "host", "slot_sums_layout.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ GPU parity
@pytest.fixture(scope="module")
def gpu_ctx():
    c = native.Context(0)
    assert "EMULATOR" not in c.describe()
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_gpu_gm17_small(gpu_ctx, curve):
    run_device_checks(gpu_ctx, curve, 7, 41, extra_public=1)
    run_device_checks(gpu_ctx, curve, 100, 44, kind="sha")


@pytest.mark.gpu
def test_gpu_gm17_two_pass(gpu_ctx):
    run_device_checks(gpu_ctx, BN254, 700, 45)        # D = 2048: cols + rows passes


@pytest.mark.gpu
def test_gpu_gm17_errors(gpu_ctx):
    run_error_checks(gpu_ctx)


@pytest.mark.gpu
def test_gpu_gm17_batch_longer_than_the_slots(gpu_ctx):
    run_long_batch_checks(gpu_ctx)


@pytest.mark.gpu
def test_gpu_gm17_config5_full_size(gpu_ctx):
    """BASELINE.json configs[4] at full size (2^20 - 2 constraints, BN254; SAP domain 2^21, ~2^21 variables) through
    size-independent properties: the proof satisfies both verification equations under the key's own vk, it depends
    on (d1, d2, r) only through r + d1, the pipelined batch equals isolated calls, and a different public input is rejected."""
    from zokrates_amd import synth
    curve = BN254
    circ = synth.circuit(0, 20)
    cs = native.ConstraintSystem(gpu_ctx, 0, circ.n, circ.l, circ.w, circ.mats())
    tox = synth.toxic_waste(0)
    raw = native.setup_gm17(gpu_ctx, cs, (tox[0], tox[1], tox[2], tox[4]))
    pk = native.ProvingKey(gpu_ctx, 0, raw, scheme="gm17")
    assert pk.hlen - 1 == 1 << 21 and pk.m == 1 + 2 + circ.w + circ.n
    vk = gm17.vk_from_pk_bytes(curve, raw)
    z = circ.assignment(0x5EED0001)
    x = int.from_bytes(z[32:64].tobytes(), "little")
    d1, d2, r_ = 0x123456789abcdef0123456789, 0xfedcba9876543210, 0x1111222233334444555566667777
    p1 = native.prove_gm17(gpu_ctx, pk, cs, z, d1, d2, r_)
    assert p1[-3:] == b"\0\0\0"
    from oracle import cpu
    # the oracle at this size: the closed form from the toxic waste (no transform, no MSM) and — ZKHIP_TEST_FULL_O2=0 skips it — the
    # C++ restatement of ark-gm17's create_proof over the key bytes the device made (four transforms on the doubled domain, five MSMs)
    oc = cpu.Circuit.from_csr(0, circ.n, circ.l, circ.w, circ.mats())
    tb = b"".join(int(v).to_bytes(32, "little") for v in (tox[0], tox[1], tox[2], tox[4]))
    assert cpu.gm17_trapdoor(oc, tb, z, d1, r_) == p1
    if os.environ.get("ZKHIP_TEST_FULL_O2", "1") != "0":
        assert cpu.gm17_prove(oc, cpu.Gm17ProvingKey.parse(0, raw), z, d1, d2, r_)[0] == p1
    del raw, oc
    assert gm17.verify(curve, vk, formats.proof_from_raw(curve, p1), [x])
    assert not gm17.verify(curve, vk, formats.proof_from_raw(curve, p1), [(x + 1) % curve.r])
    assert native.prove_gm17(gpu_ctx, pk, cs, z, d1 + 77, 5, r_ - 77) == p1
    za = native.Assignment(gpu_ctx, cs, z)
    zb = native.Assignment(gpu_ctx, cs, circ.assignment(0x5EED0002))
    proofs, _ = native.prove_gm17_resident_batch(gpu_ctx, pk, cs, [za, zb, za], [(d1, d2, r_), (1, 2, 3), (d1, 0, r_)])
    assert proofs[0] == p1 and proofs[2] == p1 and proofs[1] == native.prove_gm17(gpu_ctx, pk, cs, zb, 1, 2, 3)
    assert proofs[1] != p1


# ------------------------------------------------------------------ C++ restatement (the timed CPU baseline) vs python
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_cpp_oracle_matches_python(curve):
    """oracle/c/gm17.hpp (ark-gm17's setup / create_proof / closed form in C++) is pinned bit-for-bit against
    oracle/gm17.py: key bytes, proof bytes, closed form — with extra public inputs so the f_i rows are exercised."""
    from oracle import cpu
    for n, extra, seed in ((9, 0, 51), (14, 2, 52)):
        cs, z = circuit(curve, n, seed, extra_public=extra)
        tox = gm17.Toxic.from_seed(curve, seed=seed)
        oc = cpu.Circuit.from_csr(curve.curve_id, cs.n, cs.l, cs.w, [csr_of(cs.A), csr_of(cs.B), csr_of(cs.C)])
        tb = cpu.gm17_toxic_bytes(tox)
        cpk = cpu.Gm17ProvingKey.setup(oc, tb)
        opk, ovk = gm17.setup(curve, cs, tox)
        raw = cpk.serialize()
        assert raw.tobytes() == gm17.pk_serialize(curve, opk)
        assert cpu.Gm17ProvingKey.parse(curve.curve_id, raw).serialize().tobytes() == raw.tobytes()
        rnd = random.Random(seed)
        d1, d2, r_ = (rnd.randrange(curve.r) for _ in range(3))
        got, _ = cpu.gm17_prove(oc, cpk, le(z), d1, d2, r_)
        assert got == proof_bytes(curve, gm17.prove(curve, cs, opk, z, d1, d2, r_))
        assert got == cpu.gm17_trapdoor(oc, tb, le(z), d1, r_)
        assert cpu.gm17_trapdoor(oc, tb, le(z), 0, 0) == proof_bytes(curve, gm17.trapdoor_prove(curve, cs, tox, z, 0, 0))


@pytest.mark.gpu
def test_gpu_gm17_vs_cpp_oracle_mid_size(gpu_ctx):
    """2^14 constraints (SAP domain 2^15, two-pass NTT, c = 10 windows): device key bytes and proof == C++ oracle."""
    from oracle import cpu
    from zokrates_amd import synth
    for curve_id, lg in ((0, 14), (1, 12)):
        circ = synth.circuit(curve_id, lg, seed=0x77 + lg)
        z = circ.assignment(0x5EED0003)
        cs = native.ConstraintSystem(gpu_ctx, curve_id, circ.n, circ.l, circ.w, circ.mats())
        tox = synth.toxic_waste(curve_id)
        t4 = (tox[0], tox[1], tox[2], tox[4])
        raw = native.setup_gm17(gpu_ctx, cs, t4)
        oc = cpu.Circuit.from_csr(curve_id, circ.n, circ.l, circ.w, circ.mats())
        tb = b"".join(int(v).to_bytes(32, "little") for v in t4)
        cpk = cpu.Gm17ProvingKey.setup(oc, tb)
        assert cpk.serialize().tobytes() == raw.tobytes()
        pk = native.ProvingKey(gpu_ctx, curve_id, raw, scheme="gm17")
        d1, d2, r_ = 0x1234567890abcdef1234567890, 0xdeadbeef, 0x55556666777788889999
        want, _ = cpu.gm17_prove(oc, cpk, z, d1, d2, r_)
        assert want == cpu.gm17_trapdoor(oc, tb, z, d1, r_)
        assert native.prove_gm17(gpu_ctx, pk, cs, z, d1, d2, r_) == want


# ------------------------------------------------------------------ the reference's own golden vector
def _golden_triple():
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gm17_bls12_377_triple.json")
    d = json.load(open(path))
    h = lambda s: int(s, 16)
    g1 = lambda p: (h(p[0]), h(p[1]))
    g2 = lambda p: ((h(p[0][0]), h(p[0][1])), (h(p[1][0]), h(p[1][1])))
    vk = d["vk"]
    ovk = dict(h_g2=g2(vk["h"]), g_alpha_g1=g1(vk["g_alpha"]), h_beta_g2=g2(vk["h_beta"]), g_gamma_g1=g1(vk["g_gamma"]),
               h_gamma_g2=g2(vk["h_gamma"]), query=[g1(p) for p in vk["query"]])
    proof = (g1(d["proof"]["a"]), g2(d["proof"]["b"]), g1(d["proof"]["c"]))
    return d, ovk, proof, [h(v) for v in d["inputs"]]


def test_reference_golden_triple_verifies():
    """The only (proof, verification key, inputs) triple the reference holds for a pairing-based scheme
    (/root/reference/zokrates_stdlib/tests/tests/snark/gm17.json, produced by the reference's own ark GM17 backend over
    BLS12-377, expected `true`) satisfies the oracle's restatement of the two GM17 verification equations — this pins
    `gm17.verify` (equation shape, G2 JSON layout [[x.c0, x.c1], [y.c0, y.c1]], big-endian hex, query[0] + sum x_i
    query[i]) on a reference artefact; any perturbation is rejected."""
    from oracle.fields import BLS12_377
    d, vk, proof, inputs = _golden_triple()
    assert d["expected"] is True and len(vk["query"]) == len(inputs) + 1
    assert vk["h_g2"] == vk["h_gamma_g2"]                      # gamma = 1: ark's generate_random_parameters
    assert gm17.verify_embedded(BLS12_377, vk, proof, inputs)
    assert not gm17.verify_embedded(BLS12_377, vk, proof, [inputs[0], inputs[1], inputs[2] + 1])
    swapped = (proof[0], (proof[1][0][::-1], proof[1][1][::-1]), proof[2])      # [c1, c0] is not the encoding
    with pytest.raises(Exception):
        assert gm17.verify_embedded(BLS12_377, vk, swapped, inputs)


def test_embedded_and_native_verification_agree():
    curve = BN254
    cs, z = circuit(curve, 5, 23)
    tox = gm17.Toxic.from_seed(curve)
    pk, vk = gm17.setup(curve, cs, tox)
    proof = gm17.prove(curve, cs, pk, z, 4, 5, 6)
    assert gm17.verify(curve, vk, proof, z[1:cs.l]) and gm17.verify_embedded(curve, vk, proof, z[1:cs.l])
    bad = (proof[0], proof[1], pk["g_gamma_z"])
    assert not gm17.verify(curve, vk, bad, z[1:cs.l]) and not gm17.verify_embedded(curve, vk, bad, z[1:cs.l])


def test_reference_embed_triples_verify():
    """Three more reference artefacts (zokrates_core_test/tests/tests/snark/snark_verify_bls12_377_{1,2,5}.json: GM17
    proofs made with `zokrates setup/generate-proof -b ark -s gm17` over BLS12-377, with 1, 2 and 5 public inputs) pass
    the oracle's GM17 verification; a wrong input fails."""
    import json
    from oracle.fields import BLS12_377
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gm17_bls12_377_embed_triples.json")
    doc = json.load(open(path))
    assert len(doc["triples"]) == 3
    for t in doc["triples"]:
        p, v = [int(x) for x in t["proof"]], [int(x) for x in t["vk"]]
        inputs = [int(x) for x in t["inputs"]]
        g1 = lambda a, i: (a[i], a[i + 1])
        g2 = lambda a, i: ((a[i], a[i + 1]), (a[i + 2], a[i + 3]))
        proof = (g1(p, 0), g2(p, 2), g1(p, 6))
        vk = dict(h_g2=g2(v, 0), g_alpha_g1=g1(v, 4), h_beta_g2=g2(v, 6), g_gamma_g1=g1(v, 10), h_gamma_g2=g2(v, 12),
                  query=[g1(v, 16 + 2 * i) for i in range(len(inputs) + 1)])
        assert gm17.verify_embedded(BLS12_377, vk, proof, inputs), t["source"]
        assert not gm17.verify_embedded(BLS12_377, vk, proof, [inputs[0] + 1] + inputs[1:]), t["source"]


# ------------------------------------------------------------------ one GM17 proof across several GPUs (virtual ranks)
def _gm17_sharded_checks(ctx, curve, world, n=21, seed=61):
    from oracle import cpu
    cs, z = circuit(curve, n, seed, extra_public=1)
    tox = gm17.Toxic.from_seed(curve)
    mats = [csr_of(cs.A), csr_of(cs.B), csr_of(cs.C)]
    dcs = native.ConstraintSystem(ctx, curve.curve_id, cs.n, cs.l, cs.w, mats)
    oc = cpu.Circuit.from_csr(curve.curve_id, cs.n, cs.l, cs.w, mats)
    tb = cpu.gm17_toxic_bytes(tox)
    raw = cpu.Gm17ProvingKey.setup(oc, tb).serialize()
    zb = le(z)
    d1, d2, r_ = 0xabcdef12345 % curve.r, 99, 0x13579bdf2468 % curve.r
    want = cpu.gm17_trapdoor(oc, tb, zb, d1, r_)
    shards = [native.ProvingKey(ctx, curve.curve_id, raw, rank=k, world=world, scheme="gm17") for k in range(world)]
    parts = [native.prove_gm17_partial(ctx, shards[k], dcs, zb, d1, d2, r_) for k in range(world)]
    assert native.combine_gm17(ctx, shards[0], parts, d1, d2, r_) == want
    assert native.combine_gm17(ctx, shards[-1], parts[::-1], d1, d2, r_) == want        # order and combining rank do not matter
    za = native.Assignment(ctx, dcs, zb)
    parts = [native.prove_gm17_partial(ctx, shards[k], dcs, za, 0, 0, 0) for k in range(world)]
    assert native.combine_gm17(ctx, shards[0], parts, 0, 0, 0) == cpu.gm17_trapdoor(oc, tb, zb, 0, 0)
    with pytest.raises(native.ZkhipError):                                              # a shard cannot prove alone
        native.prove_gm17(ctx, shards[0], dcs, zb, d1, d2, r_)
    with pytest.raises(native.ZkhipError):                                              # nor be combined as a Groth16 key
        native.combine_g16(ctx, shards[0], parts, 1, 2)
    whole = native.ProvingKey(ctx, curve.curve_id, raw, scheme="gm17")
    assert native.combine_gm17(ctx, whole, [native.prove_gm17_partial(ctx, whole, dcs, zb, d1, d2, r_)], d1, d2, r_) == want
    # a shard's key image keeps its range
    sh2 = native.ProvingKey.from_image(ctx, curve.curve_id, shards[1].export_image(), scheme="gm17")
    p_img, p_ref = (native.prove_gm17_partial(ctx, k, dcs, zb, d1, d2, r_) for k in (sh2, shards[1]))
    parts = [native.prove_gm17_partial(ctx, shards[k], dcs, zb, d1, d2, r_) for k in range(world)]
    assert native.combine_gm17(ctx, shards[0], [parts[0], p_img] + parts[2:], d1, d2, r_) == want
    # partial records are canonical (affine, ZZ = ZZZ = 1): the same share gives the same bytes, whatever order the
    # bucket sort's atomics placed the points in
    assert p_img.tobytes() == p_ref.tobytes() == parts[1].tobytes()


@pytest.mark.parametrize("curve,world", [(BN254, 2), (BN254, 5), (BLS12_381, 3)], ids=lambda v: getattr(v, "name", str(v)))
def test_emu_gm17_sharded_virtual_ranks(emu_ctx, curve, world):
    _gm17_sharded_checks(emu_ctx, curve, world)


def test_emu_gm17_more_ranks_than_points(emu_ctx):
    _gm17_sharded_checks(emu_ctx, BN254, 9, n=3)     # most ranks own an empty range


@pytest.mark.gpu
def test_gpu_gm17_sharded_virtual_ranks(gpu_ctx):
    _gm17_sharded_checks(gpu_ctx, BN254, 4, n=300)
    _gm17_sharded_checks(gpu_ctx, BLS12_381, 3, n=100)
