"""BLS12-377, the third curve libzkhip proves over (curve id 2): Groth16 and GM17 against a Python big-int reference.

No C++ oracle exists for this curve, so the reference is tests/bls377_ref.py: the oracle's curve-agnostic parts (QAP / SAP at the
trapdoor, closed-form proof scalars, the algorithmic provers, the byte formats, the pairing) over an Fq2 with u^2 = -5.
CPU tests run on the emulator build; the `gpu` ones repeat them on the device and add the sizes only a device reaches."""
import json
import os
import random
import subprocess
import time

import numpy as np
import pytest

import bls377_ref as ref
from oracle import formats, ir, pairing
from oracle import gm17 as ogm17
from oracle import groth16 as g16
from zokrates_amd import native, synth

from emu_util import EMU_DIR, EMU_LIB, emu_library

C = ref.CURVE
CID = 2
G1, G2 = ref.groups377()
HERE = os.path.dirname(os.path.abspath(__file__))


def le(vals, nb=32):
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "little") for v in vals), dtype=np.uint8)


def pts1(ps):
    return np.frombuffer(b"".join(formats.ser_g1(C, P) for P in ps), dtype=np.uint8)


def pts2(ps):
    return np.frombuffer(b"".join(formats.ser_g2(C, P) for P in ps), dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0, emu_library())
    assert "EMULATOR" in c.describe()
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu_ctx():
    c = native.Context(0)
    assert "gfx950" in c.describe() and "EMULATOR" not in c.describe()
    yield c
    c.close()


# ------------------------------------------------------------------ constants
def test_constants():
    """The constants of the curve as the library and the tests write them down: generators on their curves and of order r, -5 a
    non-residue, the twist coefficient 1 / u, the two-adic root, the program-file id."""
    r, q = C.r, C.q
    assert r.bit_length() == 253 and q.bit_length() == 377 and (r - 1) % (1 << 47) == 0 and (r - 1) % (1 << 48) != 0
    assert pow(22, (r - 1) // 2, r) == r - 1 and pow(22, (r - 1) >> 47, r) == C.two_adic_root
    assert pow(q - ref.BETA, (q - 1) // 2, q) == q - 1
    assert ref.F2.mul(C.b2, (0, 1)) == (1, 0)
    assert G1.on_curve(C.g1) and G2.on_curve(C.g2)
    assert G1.amul(C.g1, r) is None and G2.amul(C.g2, r) is None
    assert synth.FR_MODULUS[CID] == r and native.CURVE_IDS["bls12_377"] == CID and native.FQ_BYTES[CID] == 48


# ------------------------------------------------------------------ 1. field operations
def _field_ops(c):
    rnd = random.Random(377)
    for field, p, nb in ((0, C.r, 32), (1, C.q, 48)):
        a = [0, 1, p - 1, p - 1, 2, (1 << (8 * nb)) % p] + [rnd.randrange(p) for _ in range(70)]
        b = [0, p - 1, p - 1, 1, p - 2, (1 << (8 * nb)) % p] + [rnd.randrange(p) for _ in range(70)]
        for op, fn in (("add", lambda x, y: (x + y) % p), ("sub", lambda x, y: (x - y) % p), ("mul", lambda x, y: x * y % p)):
            got = c.field_op(CID, field, op, le(a, nb), le(b, nb))
            assert got.tobytes() == le([fn(x, y) for x, y in zip(a, b)], nb).tobytes(), (field, op)


def _fq2_ops(c, curve_id=CID, F2=ref.F2):
    """Fq2 in the saturated form (field 2) and in the MSM kernels' unsaturated limbs (field 3: the inlined hot forms with loose
    quotient digits, the out-of-line ones, the fused a b - a a of the mixed addition), operands 0, 1, u, q - 1 and random."""
    q = F2.q
    rnd = random.Random(378)
    edge = [(0, 0), (1, 0), (0, 1), (q - 1, q - 1), (q - 1, 0), (0, q - 1), (1, q - 1), (q - 1, 1), (2, 3)]
    a = [x for x in edge for _ in edge] + [(rnd.randrange(q), rnd.randrange(q)) for _ in range(60)]
    b = [y for _ in edge for y in edge] + [(rnd.randrange(q), rnd.randrange(q)) for _ in range(60)]
    pack = lambda xs: le([v for x in xs for v in x], 48 if q.bit_length() > 256 else 32)
    sqr = lambda x, y: F2.mul(x, x)
    ops = [("add", F2.add), ("sub", F2.sub), ("mul", F2.mul), ("sqr", sqr), ("inv", lambda x, y: F2.inv(x) if x != (0, 0) else (0, 0))]
    hot = [("mul_call", F2.mul), ("sqr_call", sqr), ("mulsub", lambda x, y: F2.sub(F2.mul(x, y), F2.mul(x, x)))]
    k = lambda n, x: (n * x[0] % q, n * x[1] % q)
    # the hot forms on un-reduced multiples 3a (< 6p) and 4b (< 8p): the upper end of the operand values they are written for
    hot += [("mul_wide", lambda x, y: F2.mul(k(3, x), k(4, y))), ("sqr_wide", lambda x, y: F2.mul(k(3, x), k(3, x))),
            ("mulsub_wide", lambda x, y: F2.sub(F2.mul(k(3, x), k(4, y)), F2.mul(k(3, x), k(4, x))))]
    for field, table in ((2, ops), (3, ops + hot)):
        for op, fn in table:
            got = c.field_op(curve_id, field, op, pack(a), pack(b))
            want = pack([fn(x, y) for x, y in zip(a, b)])
            assert got.tobytes() == want.tobytes(), (field, op)


def test_field_ops(ctx):
    _field_ops(ctx)


def test_fq2_ops(ctx):
    _fq2_ops(ctx)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_fq2_ops_of_the_other_curves_are_unchanged(ctx, curve_id):
    """The same entry point over u^2 = -1: the non-residue is a property of the field's parameter pack."""
    from oracle.fields import BLS12_381, BN254
    _fq2_ops(ctx, curve_id, ref.Fq2Beta((BN254, BLS12_381)[curve_id].q, 1))


# ------------------------------------------------------------------ 2. transforms
def _ntt(c, logns):
    rnd = random.Random(379)
    for logn in logns:
        n = 1 << logn
        dom = g16.Domain(C, n)
        a = [rnd.randrange(C.r) for _ in range(n)]
        for d, fn in (("fft", dom.fft), ("ifft", dom.ifft), ("coset_fft", dom.coset_fft), ("coset_ifft", dom.coset_ifft)):
            assert c.ntt(CID, le(a), d).tobytes() == le(fn(a)).tobytes(), (logn, d)


def test_ntt(ctx):
    """2^0 ... 2^10, both directions, plain and on the coset, against oracle.groth16.Domain (roots from a two-adicity of 47)."""
    _ntt(ctx, range(0, 11))


def test_ntt_two_passes():
    c2 = native.Context(0, emu_library())
    try:
        c2.tune("ntt_single_max_log", 1)
        _ntt(c2, (2, 3, 5, 6, 7))
    finally:
        c2.close()


# ------------------------------------------------------------------ 3. multi-scalar multiplication
def _golden_g2(golden_dir):
    """G2 points the reference itself made on this twist: h, h_beta, h_gamma of its GM17 verification keys."""
    out = []
    def walk(o):
        if isinstance(o, dict):
            for k, v in o.items():
                if k in ("h", "h_beta", "h_gamma", "h_g2", "h_beta_g2", "h_gamma_g2") and isinstance(v, list) and len(v) == 2 and isinstance(v[0], list):
                    out.append(((int(v[0][0], 16), int(v[0][1], 16)), (int(v[1][0], 16), int(v[1][1], 16))))
                else:
                    walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)
    for name in ("gm17_bls12_377_triple.json", "gm17_bls12_377_embed_triples.json"):
        walk(json.load(open(os.path.join(golden_dir, name))))
    assert out
    return out


def _msm_case(rnd, n, golden):
    p1 = [G1.amul(G1.gen, rnd.randrange(1, C.r)) for _ in range(n)]
    p2 = [G2.amul(G2.gen, rnd.randrange(1, C.r)) for _ in range(n)]
    for i, Q in enumerate(golden[:n // 2]):
        p2[n - 1 - i] = Q
    ks = [rnd.randrange(C.r) for _ in range(n)]
    if n >= 8:
        ks[0] = 0; ks[1] = 1; ks[2] = C.r - 1
        p1[3] = None; p2[4] = None
        p1[5] = p1[6]; ks[5] = ks[6]
        p2[5] = p2[6]
        p1[7] = G1.aneg(p1[6]); p2[7] = G2.aneg(p2[6]); ks[7] = ks[6]
    return p1, p2, ks


def _msm(c, sizes, golden):
    rnd = random.Random(380)
    for n in sizes:
        p1, p2, ks = _msm_case(rnd, n, golden)
        want1, want2 = G1.to_affine(G1.msm(p1, ks)), G2.to_affine(G2.msm(p2, ks))
        got1, got2 = c.msm(CID, 1, pts1(p1), le(ks)), c.msm(CID, 2, pts2(p2), le(ks))
        assert got1[-1] == 0 and got1[:96] == formats.ser_g1(C, want1), n
        assert got2[-1] == 0 and got2[:192] == formats.ser_g2(C, want2), n
    assert c.msm(CID, 1, pts1(p1)[:0], le(ks)[:0])[-1] == 1
    assert c.msm(CID, 2, pts2(p2), np.zeros_like(le(ks)))[-1] == 1
    Q = golden[0]                                             # Q - Q: the sum is the point at infinity
    assert c.msm(CID, 2, pts2([Q, G2.aneg(Q)]), le([5, 5]))[-1] == 1


def test_golden_g2_points_are_on_the_twist(golden_dir):
    for Q in _golden_g2(golden_dir):
        assert G2.on_curve(Q) and G2.amul(Q, C.r) is None


def test_msm(ctx, golden_dir):
    _msm(ctx, (1, 3, 20, 45), _golden_g2(golden_dir))


def test_msm_window_sizes(ctx, golden_dir):
    rnd = random.Random(381)
    p1, p2, ks = _msm_case(rnd, 24, _golden_g2(golden_dir))
    want1 = formats.ser_g1(C, G1.to_affine(G1.msm(p1, ks)))
    want2 = formats.ser_g2(C, G2.to_affine(G2.msm(p2, ks)))
    try:
        for c in (2, 3, 5, 8, 13, 16, 17):
            ctx.tune("msm_c", c)
            assert ctx.msm(CID, 1, pts1(p1), le(ks))[:96] == want1, c
            if c in (3, 8, 13):
                assert ctx.msm(CID, 2, pts2(p2), le(ks))[:192] == want2, c
    finally:
        ctx.tune("msm_c", 0)


# ------------------------------------------------------------------ 4. Groth16 and GM17
def _system(c, n, kind, seed=0x377):
    cs, z = g16.synthetic_chain(C, n, seed, kind)
    assert cs.is_satisfied(z, C.r)
    return cs, z, native.ConstraintSystem(c, CID, cs.n, cs.l, cs.w, ref.csr(cs))


def _tox5(t):
    return (t.alpha, t.beta, t.gamma, t.delta, t.tau)


def _g16_everywhere(c, n, kind, algorithmic=True, verify=True, members=3):
    cs, z, ncs = _system(c, n, kind)
    zb = le(z)
    tox = g16.Toxic.from_seed(C)
    raw = native.setup_g16(c, ncs, _tox5(tox))
    if algorithmic:
        opk, _ = ref.g16_setup(cs, tox)
        assert raw.tobytes() == formats.ark_pk_serialize(C, opk), "device setup differs from the reference's key"
    rs = [(0x1234567, 0x89abcdef0123), (5, 6), (0, 7), (1 << 200, 0)]
    want = [formats.proof_raw(C, ref.g16_trapdoor(cs, tox, z, a, b)) for a, b in rs]
    if algorithmic:
        assert formats.proof_raw(C, ref.g16_prove(cs, opk, z, *rs[0])) == want[0]
    pk = native.ProvingKey(c, CID, raw)
    assert (pk.m, pk.w, pk.l) == (cs.m, cs.w, cs.l)
    assert ncs.witness_map(zb).tobytes() == le(g16.witness_map(C, cs, z)).tobytes()
    for bound in (False, True):
        if bound:
            pk.bind(ncs)
            assert pk.is_bound(ncs)
        assert [native.prove_g16(c, pk, ncs, zb, a, b) for a, b in rs] == want, bound       # lone
        za = native.Assignment(c, ncs, zb)
        assert native.prove_g16_resident(c, pk, ncs, za, *rs[1]) == want[1], bound          # resident
        proofs, _ = native.prove_g16_resident_batch(c, pk, ncs, [za] * len(rs), rs)         # resident batch
        assert proofs == want, bound
        proofs, _ = native.prove_g16_batch(c, pk, ncs, np.concatenate([zb] * len(rs)), rs)  # batch from host memory
        assert proofs == want, bound
        za.close()
    image = pk.export_image()                                                               # key image round trip (of the bound key)
    pk2 = native.ProvingKey.from_image(c, CID, image)
    assert native.prove_g16(c, pk2, ncs, zb, *rs[0]) == want[0]
    pk2.close()
    pk.unbind()
    assert native.prove_g16(c, pk, ncs, zb, *rs[0]) == want[0]
    shards = [native.ProvingKey(c, CID, raw, rank=k, world=members) for k in range(members)]   # one proof over three members
    parts = [native.prove_g16_partial(c, shards[k], ncs, zb, *rs[0]) for k in range(members)]
    assert native.combine_g16(c, shards[0], parts, *rs[0]) == want[0]
    assert native.combine_g16(c, shards[-1], parts[::-1], *rs[0]) == want[0]
    if verify:
        vk = formats.ark_pk_deserialize(C, raw.tobytes())["vk"]
        proof = formats.proof_from_raw(C, want[0])
        assert pairing.groth16_verify(C, vk, proof, z[1:cs.l])
        assert not pairing.groth16_verify(C, vk, proof, [(z[1] + 1) % C.r])
    for k in shards + [pk]:
        k.close()
    return raw, want[0], z[1:cs.l]


def _gm17_everywhere(c, n, kind, algorithmic=True, verify=True, members=3):
    cs, z, ncs = _system(c, n, kind)
    zb = le(z)
    tox = ogm17.Toxic.from_seed(C)
    raw = native.setup_gm17(c, ncs, (tox.alpha, tox.beta, tox.gamma, tox.t))
    if algorithmic:
        opk, _ = ref.gm17_setup(cs, tox)
        assert raw.tobytes() == ogm17.pk_serialize(C, opk), "device GM17 setup differs from the reference's key"
    rnds = [(21, 22, 23), (0, 5, 1 << 199), (7, 0, 0)]
    want = [formats.proof_raw(C, ref.gm17_trapdoor(cs, tox, z, d1, r_)) for d1, _, r_ in rnds]
    if algorithmic:
        assert formats.proof_raw(C, ref.gm17_prove(cs, opk, z, *rnds[0])) == want[0]
    pk = native.ProvingKey(c, CID, raw, scheme="gm17")
    for bound in (False, True):
        if bound:
            pk.bind(ncs)
            assert pk.is_bound(ncs)
        assert [native.prove_gm17(c, pk, ncs, zb, *t) for t in rnds] == want, bound
        za = native.Assignment(c, ncs, zb)
        assert native.prove_gm17(c, pk, ncs, za, *rnds[1]) == want[1], bound
        proofs, _ = native.prove_gm17_resident_batch(c, pk, ncs, [za] * len(rnds), rnds)
        assert proofs == want, bound
        za.close()
    pk2 = native.ProvingKey.from_image(c, CID, pk.export_image(), scheme="gm17")
    assert native.prove_gm17(c, pk2, ncs, zb, *rnds[0]) == want[0]
    pk2.close()
    pk.unbind()
    shards = [native.ProvingKey(c, CID, raw, rank=k, world=members, scheme="gm17") for k in range(members)]
    parts = [native.prove_gm17_partial(c, shards[k], ncs, zb, *rnds[0]) for k in range(members)]
    assert native.combine_gm17(c, shards[0], parts, *rnds[0]) == want[0]
    if verify:
        vk = ogm17.vk_from_pk_bytes(C, raw)
        proof = formats.proof_from_raw(C, want[0])
        assert ogm17.verify_embedded(C, vk, proof, z[1:cs.l])
        assert not ogm17.verify_embedded(C, vk, proof, [(z[1] + 1) % C.r])
    for k in shards + [pk]:
        k.close()
    return raw, want[0], z[1:cs.l]


def _compiled_verifier(tmp_path, scheme, raw, proof_raw, inputs):
    """`zkhip-cli verify` (csrc/host/verify.cpp, the compiled host layer) on the same proof: PASSED, and FAILED with one input changed."""
    from zokrates_amd import formats as zformats
    vk = zformats.verification_key_json(CID, raw) if scheme == "g16" else zformats.verification_key_json_gm17(CID, raw)
    assert json.loads(vk)["curve"] == "bls12_377"
    (tmp_path / "verification.key").write_text(vk)
    good = zformats.proof_json(CID, proof_raw, list(inputs), scheme=scheme)
    bad = zformats.proof_json(CID, proof_raw, [(inputs[0] + 1) % C.r] + list(inputs[1:]), scheme=scheme)
    emu_library()
    env = dict(os.environ, ZKHIP_LIBRARY=EMU_LIB)
    for name, doc, verdict in (("good.json", good, "PASSED"), ("bad.json", bad, "FAILED")):
        (tmp_path / name).write_text(doc)
        r = subprocess.run([os.path.join(EMU_DIR, "zkhip-cli-emu"), "verify", "-v", str(tmp_path / "verification.key"), "-j", str(tmp_path / name)],
                           capture_output=True, text=True, env=env)
        assert r.stdout.split()[-1] == verdict, (name, r.stdout, r.stderr)


@pytest.mark.parametrize("kind,n", [("dense", 40), ("sha", 150)])
def test_groth16(ctx, tmp_path, kind, n):
    """Setup bytes == the reference's serialized key; the proof == the closed-form trapdoor proof == the algorithmic prover, byte for
    byte, through lone / resident / batch, bound and unbound key, the key image and three members; the pairing accepts it and
    rejects it with one input changed, and so does the compiled verifier."""
    raw, proof, inputs = _g16_everywhere(ctx, n, kind)
    _compiled_verifier(tmp_path, "g16", raw, proof, inputs)


@pytest.mark.parametrize("kind,n", [("dense", 40), ("sha", 100)])
def test_gm17(ctx, tmp_path, kind, n):
    raw, proof, inputs = _gm17_everywhere(ctx, n, kind)
    _compiled_verifier(tmp_path, "gm17", raw, proof, inputs)


def test_setup_without_generators_uses_the_standard_ones(ctx):
    """alpha_g1 of a key made without explicit generators is alpha times the G1 generator written down in core.cuh."""
    cs, z, ncs = _system(ctx, 5, "dense")
    tox = g16.Toxic.from_seed(C, 3)
    raw = native.setup_g16(ctx, ncs, _tox5(tox)).tobytes()
    assert raw[:96] == formats.ser_g1(C, G1.amul(C.g1, tox.alpha))
    assert raw[96:288] == formats.ser_g2(C, G2.amul(C.g2, tox.beta))


# ------------------------------------------------------------------ 5. the reference's backend unit test, on its own curve
def _reference_backend_test(c, scheme):
    """/root/reference/zokrates_ark/src/groth16.rs:123-161 and gm17.rs:124-160 run over BLS12-377: the program `(1) * (_0) == ~out_0`
    with `_0` a public argument, input 42: `out` bytes -> zkhip_prog_open -> setup -> prove -> verify."""
    prog = ir.Prog(C, [ir.Parameter(1, False)], [ir.Constraint([(0, 1)], [(1, 1)], [(-1, 1)])], return_count=1)
    data = ir.serialize_prog(prog)
    assert data[8:12] == ref.PROGRAM_FILE_ID
    p = native.Program(data, c.lib)
    assert p.curve_id == CID and (p.n, p.l, p.w) == (1, 3, 0) and list(p.variable_order()) == [0, 1, -1]
    z, inputs = p.assignment(ir.serialize_witness({0: 1, 1: 42, -1: 42}))
    inp = [int.from_bytes(inputs[32 * i:32 * i + 32].tobytes(), "little") for i in range(2)]
    assert inp == [42, 42]
    cs = p.constraint_system(c)
    tox = g16.Toxic.from_seed(C, 0xBEEF)
    if scheme == "g16":
        raw = native.setup_g16(c, cs, _tox5(tox))
        pk = native.ProvingKey(c, CID, raw)
        assert (pk.m, pk.w, pk.l, pk.hlen) == (3, 0, 3, 3)
        proof = formats.proof_from_raw(C, native.prove_g16(c, pk, cs, z, 1111, 2222))
        vk = formats.ark_pk_deserialize(C, raw.tobytes())["vk"]
        assert pairing.groth16_verify(C, vk, proof, inp)
        assert not pairing.groth16_verify(C, vk, proof, [42, 43])
    else:
        raw = native.setup_gm17(c, cs, (tox.alpha, tox.beta, 1, tox.tau))
        pk = native.ProvingKey(c, CID, raw, scheme="gm17")
        proof = formats.proof_from_raw(C, native.prove_gm17(c, pk, cs, z, 1111, 2222, 3333))
        vk = ogm17.vk_from_pk_bytes(C, raw)
        assert vk["h_g2"] == vk["h_gamma_g2"]
        assert ogm17.verify_embedded(C, vk, proof, inp)
        assert not ogm17.verify_embedded(C, vk, proof, [42, 43])
    pk.close()


@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_reference_backend_unit_test(ctx, scheme):
    _reference_backend_test(ctx, scheme)


def test_program_header(ctx):
    """A header with the id c2955ab5 opens, is written back with the same id, and 0x12345678 is still refused — by name."""
    prog = ir.Prog(C, [ir.Parameter(1, False)], [ir.Constraint([(0, 1)], [(1, 1)], [(-1, 1)])], return_count=1)
    data = bytearray(ir.serialize_prog(prog))
    p = native.Program(bytes(data), ctx.lib)
    assert p.curve_id == CID
    cs, z, ncs = _system(ctx, 6, "dense")
    out = native.write_program(CID, cs.n, cs.m, ref.csr(cs), args=((1, False),), library=ctx.lib)
    assert bytes(out[8:12]) == ref.PROGRAM_FILE_ID and native.Program(bytes(out), ctx.lib).curve_id == CID
    data[8:12] = bytes.fromhex("12345678")
    with pytest.raises(native.ZkhipError) as e:
        native.Program(bytes(data), ctx.lib)
    assert "bn128, bls12_381 and bls12_377" in str(e.value)
    with pytest.raises(native.ZkhipError):
        ctx.ntt(3, le([1, 2]), "fft")                      # curve id 3 is still no curve


# ------------------------------------------------------------------ 6. the command-line tool, end to end
@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_cli_end_to_end(tmp_path, scheme):
    """zkhip-cli setup | generate-proof --verify | verify over the curve (the emulator build of the same executable)."""
    emu_library()
    env = dict(os.environ, ZKHIP_LIBRARY=EMU_LIB)
    exe = os.path.join(EMU_DIR, "zkhip-cli-emu")
    prog = ir.Prog(C, [ir.Parameter(1, True), ir.Parameter(2, False)], [
        ir.Constraint([(1, 1)], [(2, 1)], [(3, 1)]),
        ir.Constraint([(0, 1)], [(3, 1)], [(-1, 1)]),
    ], return_count=1)
    p = lambda name: str(tmp_path / name)
    open(p("out"), "wb").write(ir.serialize_prog(prog))
    open(p("witness"), "wb").write(ir.serialize_witness({0: 1, 1: 7, 2: 9, 3: 63, -1: 63}))
    run = lambda args: subprocess.run([exe] + args, capture_output=True, text=True, env=env)
    r = run(["setup", "-i", p("out"), "-p", p("proving.key"), "-v", p("verification.key"), "-s", scheme, "--entropy", "k377"])
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert json.load(open(p("verification.key")))["curve"] == "bls12_377"
    r = run(["generate-proof", "-i", p("out"), "-w", p("witness"), "-p", p("proving.key"), "-j", p("proof.json"), "-s", scheme, "--verify", "--entropy", "e"])
    assert r.returncode == 0 and "verified against the verification key" in r.stdout, (r.stdout, r.stderr)
    doc = json.load(open(p("proof.json")))
    assert doc["curve"] == "bls12_377" and doc["scheme"] == scheme and [int(x, 16) for x in doc["inputs"]] == [9, 63]
    assert run(["verify", "-v", p("verification.key"), "-j", p("proof.json")]).stdout.split()[-1] == "PASSED"
    doc["inputs"][0] = "0x" + (10).to_bytes(32, "big").hex()
    open(p("bad.json"), "w").write(json.dumps(doc))
    assert run(["verify", "-v", p("verification.key"), "-j", p("bad.json")]).stdout.split()[-1] == "FAILED"


# ------------------------------------------------------------------ 7. scheduling knobs
def test_schedule_invariance():
    """The knobs tests/schedule_checks.py turns for BN254 (that helper is tied to curve 0 and the C++ oracle): release order, fused or
    separate launches, slices per launch, the sort's placement pass (by the window width of the key's tables) — the bytes of a BLS12-377 proof do not move."""
    c2 = native.Context(0, emu_library())
    try:
        cs, z, ncs = _system(c2, 30, "sha", seed=0x5C4ED)
        zb = le(z)
        tox, gtox = g16.Toxic.from_seed(C), ogm17.Toxic.from_seed(C)
        raw, graw = native.setup_g16(c2, ncs, _tox5(tox)), native.setup_gm17(c2, ncs, (gtox.alpha, gtox.beta, gtox.gamma, gtox.t))
        pk, gpk = native.ProvingKey(c2, CID, raw), native.ProvingKey(c2, CID, graw, scheme="gm17")
        rs = [(11, 13), (0, 5), (7, 0), (1 << 200, 3)]
        want = [formats.proof_raw(C, ref.g16_trapdoor(cs, tox, z, a, b)) for a, b in rs]
        gwant = formats.proof_raw(C, ref.gm17_trapdoor(cs, gtox, z, 21, 23))
        def check(tag, pk=pk, gpk=gpk):
            assert native.prove_g16(c2, pk, ncs, zb, *rs[0]) == want[0], tag
            proofs, _ = native.prove_g16_batch(c2, pk, ncs, np.concatenate([zb] * len(rs)), rs)
            assert proofs == want, tag
            assert native.prove_gm17(c2, gpk, ncs, zb, 21, 22, 23) == gwant, tag
        for gate in (0, 1, 2):
            for fuse, waves in ((1, 0), (1, 3), (0, 0)):
                c2.tune("z_gate", gate); c2.tune("fuse_z", fuse); c2.tune("msm_fused_waves", waves)
                check((gate, fuse, waves))
        for c in (8, 9):     # the same key under the widest window of the one-level placement pass and the narrowest of the two-level one
            c2.tune("msm_c", c)
            check(("msm_c", c), native.ProvingKey(c2, CID, raw), native.ProvingKey(c2, CID, graw, scheme="gm17"))
    finally:
        c2.close()


def test_stream_plan_invariance():
    """schedule_checks.stream_plan_invariance for this curve: a resident prover's stream plan is placement only — lone proofs, a
    pipelined batch, a bound key and GM17 give the closed form's bytes; the plan is chosen before the first proof and refused after."""
    c2 = native.Context(0, emu_library())
    try:
        c2.tune("pipe_plan", 1)
        cs, z, ncs = _system(c2, 30, "sha", seed=0x51A7)
        zb = le(z)
        tox, gtox = g16.Toxic.from_seed(C), ogm17.Toxic.from_seed(C)
        pk = native.ProvingKey(c2, CID, native.setup_g16(c2, ncs, _tox5(tox)))
        rs = [(11, 13), (0, 5), (7, 0), (1 << 200, 3), (9, 9), (2, 1)]
        want = [formats.proof_raw(C, ref.g16_trapdoor(cs, tox, z, a, b)) for a, b in rs]
        assert native.prove_g16(c2, pk, ncs, zb, *rs[0]) == want[0]
        with pytest.raises(native.ZkhipError):
            c2.tune("pipe_plan", 0)           # the streams exist now
        proofs, _ = native.prove_g16_batch(c2, pk, ncs, np.concatenate([zb] * len(rs)), rs)
        assert proofs == want
        pk.bind(ncs)
        assert native.prove_g16(c2, pk, ncs, zb, *rs[1]) == want[1]
        proofs, _ = native.prove_g16_batch(c2, pk, ncs, np.concatenate([zb] * len(rs)), rs)
        assert proofs == want
        gpk = native.ProvingKey(c2, CID, native.setup_gm17(c2, ncs, (gtox.alpha, gtox.beta, gtox.gamma, gtox.t)), scheme="gm17")
        assert native.prove_gm17(c2, gpk, ncs, zb, 21, 22, 23) == formats.proof_raw(C, ref.gm17_trapdoor(cs, gtox, z, 21, 23))
    finally:
        c2.close()


# ------------------------------------------------------------------ the same on the device
@pytest.mark.gpu
def test_gpu_field_ops_and_transforms(gpu_ctx):
    _field_ops(gpu_ctx)
    _fq2_ops(gpu_ctx)
    _ntt(gpu_ctx, range(0, 11))
    rnd = random.Random(382)                                   # a two-pass size against the Python transform
    a = [rnd.randrange(C.r) for _ in range(1 << 14)]
    dom = g16.Domain(C, 1 << 14)
    assert gpu_ctx.ntt(CID, le(a), "coset_fft").tobytes() == le(dom.coset_fft(a)).tobytes()
    assert gpu_ctx.ntt(CID, le(dom.fft(a)), "ifft").tobytes() == le(a).tobytes()


@pytest.mark.gpu
def test_gpu_msm(gpu_ctx, golden_dir):
    golden = _golden_g2(golden_dir)
    _msm(gpu_ctx, (1, 3, 20, 300), golden)
    # 2^16 bases that are known multiples of the generators: the sum's discrete logarithm is a dot product in Fr
    rnd = random.Random(383)
    n, distinct = 1 << 16, 64
    mult = [rnd.randrange(1, C.r) for _ in range(distinct)]
    b1 = [formats.ser_g1(C, G1.amul(G1.gen, m)) for m in mult]
    b2 = [formats.ser_g2(C, G2.amul(G2.gen, m)) for m in mult]
    idx = [rnd.randrange(distinct) for _ in range(n)]
    ks = [rnd.randrange(C.r) for _ in range(n)]
    dot = sum(mult[i] * k for i, k in zip(idx, ks)) % C.r
    got1 = gpu_ctx.msm(CID, 1, np.frombuffer(b"".join(b1[i] for i in idx), dtype=np.uint8), le(ks))
    got2 = gpu_ctx.msm(CID, 2, np.frombuffer(b"".join(b2[i] for i in idx), dtype=np.uint8), le(ks))
    assert got1[:96] == formats.ser_g1(C, G1.amul(G1.gen, dot)) and got1[-1] == 0
    assert got2[:192] == formats.ser_g2(C, G2.amul(G2.gen, dot)) and got2[-1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("dense", 40), ("sha", 150)])
def test_gpu_groth16_and_gm17_small(gpu_ctx, kind, n):
    _g16_everywhere(gpu_ctx, n, kind)
    _gm17_everywhere(gpu_ctx, n, kind)
    _reference_backend_test(gpu_ctx, "g16")
    _reference_backend_test(gpu_ctx, "gm17")


@pytest.mark.gpu
def test_gpu_groth16_and_gm17_2e16(gpu_ctx):
    """2^16 constraints against the Python closed form (the trapdoor evaluation is O(n) big-int work: about 2 s for the QAP at tau
    and as much for the SAP at this size, printed below), every entry point, three members."""
    t0 = time.time()
    _g16_everywhere(gpu_ctx, (1 << 16) - 2, "dense", algorithmic=False, verify=False)
    t1 = time.time()
    _gm17_everywhere(gpu_ctx, (1 << 15) - 2, "dense", algorithmic=False, verify=False)
    print("2^16: Groth16 %.1f s, GM17 %.1f s (device + Python closed form)" % (t1 - t0, time.time() - t1))


def _synth_system(c, lg):
    circ = synth.circuit(CID, lg, kind="dense", seed=0xABCD + lg)
    z = circ.assignment(0x5EED + lg)
    return circ, z, native.ConstraintSystem(c, CID, circ.n, circ.l, circ.w, circ.mats())


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_gpu_2e20(gpu_ctx, tmp_path, scheme):
    """2^20 constraints (dense synthetic, both schemes; GM17's SAP then has 2^21 rows): the proof bytes are identical across
    lone, resident batch, bound and unbound key, and the pairing accepts them — oracle.pairing and the compiled verifier.  No C++
    oracle exists for this curve and the Python closed form is out of reach at this size, so THE PAIRING CHECK IS THE PIN here;
    byte equality with the closed form is pinned up to 2^16 above.  One step, no retries."""
    lg = 20
    circ, z, ncs = _synth_system(gpu_ctx, lg)
    tox = synth.toxic_waste(CID)
    if scheme == "g16":
        raw = native.setup_g16(gpu_ctx, ncs, tox)
        pk = native.ProvingKey(gpu_ctx, CID, raw)
        lone = lambda: native.prove_g16(gpu_ctx, pk, ncs, z, 0x123456789abcdef, 0xfedcba987654321)
        batch = lambda za: native.prove_g16_resident_batch(gpu_ctx, pk, ncs, [za, za], [(0x123456789abcdef, 0xfedcba987654321)] * 2)[0]
    else:
        raw = native.setup_gm17(gpu_ctx, ncs, (tox[0], tox[1], tox[2], tox[4]))
        pk = native.ProvingKey(gpu_ctx, CID, raw, scheme="gm17")
        lone = lambda: native.prove_gm17(gpu_ctx, pk, ncs, z, 31, 32, 33)
        batch = lambda za: native.prove_gm17_resident_batch(gpu_ctx, pk, ncs, [za, za], [(31, 32, 33)] * 2)[0]
    proof = lone()
    za = native.Assignment(gpu_ctx, ncs, z)
    assert batch(za) == [proof, proof]
    pk.bind(ncs)
    assert pk.is_bound(ncs) and lone() == proof and batch(za) == [proof, proof]
    pk.unbind()
    assert lone() == proof
    za.close()
    pk.close()
    zi = [int.from_bytes(bytes(z[32 * i:32 * i + 32]), "little") for i in range(circ.l)]
    pr = formats.proof_from_raw(C, proof)
    if scheme == "g16":
        nb = 48
        head = raw[:2 * nb + 3 * 4 * nb + 8 + circ.l * 2 * nb + 2 * 2 * nb].tobytes()
        rd = formats._Rd(head)
        vk = dict(alpha_g1=formats.de_g1(C, rd), beta_g2=formats.de_g2(C, rd), gamma_g2=formats.de_g2(C, rd), delta_g2=formats.de_g2(C, rd))
        vk["gamma_abc_g1"] = formats.de_vec(rd, lambda: formats.de_g1(C, rd))
        assert pairing.groth16_verify(C, vk, pr, zi[1:])
        assert not pairing.groth16_verify(C, vk, pr, [(zi[1] + 1) % C.r])
    else:
        vk = ogm17.vk_from_pk_bytes(C, raw)
        assert ogm17.verify_embedded(C, vk, pr, zi[1:])
        assert not ogm17.verify_embedded(C, vk, pr, [(zi[1] + 1) % C.r])
    _compiled_verifier_gpu(tmp_path, scheme, raw, proof, zi[1:])


def _compiled_verifier_gpu(tmp_path, scheme, raw, proof_raw, inputs):
    """`zkhip-cli verify` of the product build (the verifier runs on the host CPU)."""
    from zokrates_amd import formats as zformats
    exe = os.path.join(HERE, "..", "zokrates_amd", "zkhip-cli")
    vk = zformats.verification_key_json(CID, raw) if scheme == "g16" else zformats.verification_key_json_gm17(CID, raw)
    (tmp_path / "verification.key").write_text(vk)
    for name, ins, verdict in (("good.json", list(inputs), "PASSED"), ("bad.json", [(inputs[0] + 1) % C.r] + list(inputs[1:]), "FAILED")):
        (tmp_path / name).write_text(zformats.proof_json(CID, proof_raw, ins, scheme=scheme))
        r = subprocess.run([exe, "verify", "-v", str(tmp_path / "verification.key"), "-j", str(tmp_path / name)], capture_output=True, text=True)
        assert r.stdout.split()[-1] == verdict, (name, r.stdout, r.stderr)
