"""The transform domain sharded across the members of a zkhip_multi (csrc/ntt_shard.h): member k runs the outer pass
on its strip of columns and every other pass on its range of rows, one all-to-all in between.  zkhip_multi_ntt and
zkhip_multi_witness_map always shard when the plan allows it; zkhip_prove_g16_multi does so for unbound Groth16 keys behind
zkhip_multi_transform_shard.  Every comparison is byte for byte: transforms against oracle.cpu (BLS12-377: the closed forms and the
Python transform of tests/ntt_structured.py), the witness map against the oracle's, proofs against the closed form of the trapdoor —
and, at the two sizes whose oracle would take minutes, against member 0's own zkhip_ntt, which the rest of the suite holds to the
oracle.  The members share device 0, as in tests/test_multi_device.py: on one GPU they time-slice, which is how every cross-member
wait and copy runs here; the emulator runs them one after another.

The geometry itself (strips, ranges, blocks, staging, the predicate) is held on the host in tests/host/ntt_shard_layout.cpp."""
import os
import subprocess

import numpy as np
import pytest

import bls377_ref as ref
from emu_util import emu_library
from ntt_structured import DIRS, check_structured
from oracle import cpu, formats
from oracle import gm17
from oracle import groth16 as g16
from size_ladder import CURVES, le, ntt_plan, ntt_reference, uniform_fr
from zokrates_amd import native, synth

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ the rule and a group of members
def shardable(logn, G, plan):
    """the stated rule on the plan get_plan makes under the knobs `plan` (size_ladder.ntt_plan restates get_plan)"""
    p = ntt_plan(logn, **plan)
    N1, Nb = 1 << p["log1"], 1 << (p["log2"] + p["log3"])
    return G >= 2 and G & (G - 1) == 0 and p["log1"] > 0 and G <= N1 and 2 * G <= Nb


KNOBS = {"single_max": "ntt_single_max_log", "sub": "ntt_max_sublog"}
TWO_PASS = {"single_max": 1}          # two passes from 2^2 on: cols and rows passes as short as 2 and 4
THREE_PASS_3 = {"sub": 3}             # three passes from 2^7 to 2^9
THREE_PASS_4 = {"sub": 4}             # ... from 2^9 to 2^12


def members(lib, G, plan, devices=None):
    """G members (on device 0 unless told otherwise), every member's context tuned BEFORE anything is loaded"""
    multi = native.Multi(devices if devices is not None else [0] * G, lib)
    for k in range(len(multi)):
        c = multi.member_context(k)
        for name, v in plan.items():
            c.tune(KNOBS[name], v)
    return multi


# ------------------------------------------------------------------ transforms
def ntt_checks(lib, curve_id, G, logs, plan):
    """multi.ntt in four directions against cpu.ntt on one group of members; last_shard tells the rule"""
    multi = members(lib, G, plan)
    try:
        for logn in logs:
            a, want = ntt_reference(curve_id, logn)
            for d in DIRS:
                assert multi.ntt(curve_id, a, d).tobytes() == want[d], (CURVES[curve_id].name, G, logn, d)
                assert multi.last_shard() == (G if shardable(logn, G, plan) else 0), (G, logn, plan)
    finally:
        multi.close()


def ntt_against_member0(lib, curve_id, G, logn, dirs, plan={}):
    """... against member 0's zkhip_ntt (not under test: held to the oracle by tests/test_size_ladder.py), where the oracle is slow"""
    multi = members(lib, G, plan)
    try:
        assert shardable(logn, G, plan)
        a = uniform_fr(CURVES[curve_id], 1 << logn, 0x5A4D0000 + logn)
        ctx = multi.member_context(0)
        for d in dirs:
            want = ctx.ntt(curve_id, a, d).tobytes()
            assert multi.ntt(curve_id, a, d).tobytes() == want, (G, logn, d)
            assert multi.last_shard() == G
    finally:
        multi.close()


# ------------------------------------------------------------------ witness map
def witness_map_checks(lib, curve_id, G, logs, plan, kinds=("dense",)):
    """multi.witness_map against the oracle's witness map and member 0's zkhip_witness_map"""
    multi = members(lib, G, plan)
    try:
        for logn in logs:
            for kind in kinds:
                circ = synth.circuit(curve_id, logn, kind=kind, seed=0x5AAD + logn)
                z = circ.assignment(0x5EED + logn)
                oc = cpu.Circuit.from_csr(curve_id, circ.n, circ.l, circ.w, circ.mats())
                assert oc.N == 1 << logn
                want = cpu.witness_map(oc, z).tobytes()
                multi.load_constraint_system(curve_id, circ.n, circ.l, circ.w, circ.mats())
                assert multi.witness_map(z).tobytes() == want, (CURVES[curve_id].name, G, logn, kind)
                assert multi.last_shard() == (G if shardable(logn, G, plan) else 0), (G, logn, plan)
                ctx = multi.member_context(0)
                cs = native.ConstraintSystem(ctx, curve_id, circ.n, circ.l, circ.w, circ.mats())
                assert cs.witness_map(z).tobytes() == want
                cs.close()
                assert multi.witness_map(z).tobytes() == want          # ... again: the staging turns over
    finally:
        multi.close()


# ------------------------------------------------------------------ proofs
_cases = {}


def proof_case(curve_id, logn, kind="dense"):
    """(circuit dimensions and matrices, assignment, key bytes, key bytes of GM17 or None, {(r, s): expected proof}, ...) from the
    oracle alone, made once per curve and size"""
    key = (curve_id, logn, kind)
    if key not in _cases:
        if len(_cases) >= 3:
            _cases.clear()
        if curve_id == 2:
            C = ref.CURVE
            cs, z = g16.synthetic_chain(C, (1 << logn) - 2, 0x377500 + logn)
            assert cs.domain_size() == 1 << logn
            tox = g16.Toxic.from_seed(C, 0xC0FFEE + logn)
            want = lambda r, s: formats.proof_raw(C, ref.g16_trapdoor(cs, tox, z, r, s))
            # (the key is made by the library on first use — `load` —, as tests/size_ladder.py does over this curve: the expected proof is
            # the closed form of the trapdoor, which no key byte enters)
            _cases[key] = dict(dims=(cs.n, cs.l, cs.w), mats=ref.csr(cs), z=le(z), raw=None, want=want, tox=(tox.alpha, tox.beta, tox.gamma, tox.delta, tox.tau))
        else:
            circ = synth.circuit(curve_id, logn, kind=kind, seed=0x5AAD + logn)
            z = circ.assignment(0x5EED + logn)
            oc = cpu.Circuit.from_csr(curve_id, circ.n, circ.l, circ.w, circ.mats())
            tox = cpu.toxic_bytes(g16.Toxic.from_seed(CURVES[curve_id]))
            raw = cpu.ProvingKey.setup(oc, tox).serialize()
            _cases[key] = dict(dims=(circ.n, circ.l, circ.w), mats=circ.mats(), z=z, raw=raw, want=lambda r, s: cpu.trapdoor(oc, tox, z, r, s), oc=oc)
    return _cases[key]


RS = ((0x1234567890abcdef, 0xfedcba9876543210fedcba), (3, 4))


def load(multi, curve_id, case, scheme="g16", raw=None):
    n, l, w = case["dims"]
    if case["raw"] is None:
        ctx = multi.member_context(0)
        cs = native.ConstraintSystem(ctx, curve_id, n, l, w, case["mats"])
        case["raw"] = native.setup_g16(ctx, cs, case["tox"])
        cs.close()
    multi.load_constraint_system(curve_id, n, l, w, case["mats"])
    multi.load_proving_key(curve_id, case["raw"] if raw is None else raw, scheme=scheme)


def proof_checks(lib, curve_id, G, logn, plan, rccl=False, devices=None):
    """A proof with the switch on: the closed form of the trapdoor, the bytes of the switch-off proof, last_shard() == G; a second
    proof right behind it (the staging sets alternate across proofs), and off again."""
    case = proof_case(curve_id, logn)
    multi = members(lib, G, plan, devices)
    try:
        assert shardable(logn, G, plan)
        load(multi, curve_id, case)
        if rccl:
            multi.use_rccl(True)
        assert multi.transform_shard() is False and multi.last_shard() == 0          # off by default
        (r, s), (r2, s2) = RS
        want, want2 = case["want"](r, s), case["want"](r2, s2)
        off = multi.prove_g16(z := case["z"], r, s)
        assert off == want and multi.last_shard() == 0
        assert multi.transform_shard(True) is False
        assert multi.prove_g16(z, r, s) == off and multi.last_shard() == G, (CURVES[curve_id].name, G, logn, plan, rccl)
        assert multi.prove_g16(z, r2, s2) == want2 and multi.last_shard() == G
        assert multi.prove_g16(z, r, s) == off and multi.last_shard() == G
        assert not multi.last_split()
        assert multi.transform_shard(False) is True
        assert multi.prove_g16(z, r2, s2) == want2 and multi.last_shard() == 0
    finally:
        multi.close()


def fallback_checks(lib, logn, plan, one_pass_logn, many, monkeypatch):
    """What does not shard proves as before — the right proof, last_shard() == 0 — with the switch on: three members; a one-pass
    domain (2^one_pass_logn on the default plan); more members than outer indices (`many`: members, domain, plan); a bound key
    with both switches on (it keeps the a/b split); GM17."""
    r, s = RS[0]
    assert ntt_plan(one_pass_logn)["passes"] == 1 and many[0] == 2 << ntt_plan(many[1], **many[2])["log1"]          # (2 N1 members)
    for G, lg, p in ((3, logn, plan), (2, one_pass_logn, {}), many):
        assert not shardable(lg, G, p)
        case = proof_case(0, lg)
        multi = members(lib, G, p)
        try:
            load(multi, 0, case)
            multi.transform_shard(True)
            assert multi.prove_g16(case["z"], r, s) == case["want"](r, s) and multi.last_shard() == 0, (G, lg, p)
        finally:
            multi.close()
    case = proof_case(0, logn)
    want = case["want"](r, s)
    monkeypatch.setenv("ZKHIP_SPLIT_MIN_LOG", "0")          # (read when a context is made: the members below split any bound domain)
    multi = members(lib, 2, plan)
    try:
        assert shardable(logn, 2, plan)
        load(multi, 0, case)
        multi.transform_shard(True)
        multi.bind(case["raw"])
        assert multi.transform_split() is True
        assert multi.prove_g16(case["z"], r, s) == want and multi.last_shard() == 0 and multi.last_split()
        multi.unbind()
        assert multi.prove_g16(case["z"], r, s) == want and multi.last_shard() == 2 and not multi.last_split()
        tb17 = cpu.gm17_toxic_bytes(gm17.Toxic.from_seed(CURVES[0]))
        raw17 = cpu.Gm17ProvingKey.setup(case["oc"], tb17).serialize()
        load(multi, 0, case, scheme="gm17", raw=raw17)
        assert multi.prove_gm17(case["z"], 5, 6, 7) == cpu.gm17_trapdoor(case["oc"], tb17, case["z"], 5, 7) and multi.last_shard() == 0
    finally:
        multi.close()


# ================================================================== host
def test_ntt_shard_layout_host(tmp_path):
    """tests/host/ntt_shard_layout.cpp under ASan + UBSan, a stand-alone program on the CPU: the one geometry function of every member"""
    exe = str(tmp_path / "ntt_shard_layout")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_EMU", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(HERE, "..", "zokrates_amd", "csrc"),
                           os.path.join(HERE, "host", "ntt_shard_layout.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr


# ================================================================== emulator
EMU_TWO_PASS_LOGS = tuple(range(3, 9))          # N1 x Nb from 2 x 4 to 16 x 16: G = N1, 2 G = Nb and one row per range among them
EMU_THREE_PASS_LOGS = (7, 8, 9)


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("curve_id", [0, 1], ids=["bn254", "bls12_381"])
def test_emu_ntt_two_pass(curve_id, G):
    assert shardable(3, 2, TWO_PASS) and not shardable(3, 4, TWO_PASS) and shardable(5, 4, TWO_PASS)          # (2 x 4: G = N1 = Nb / 2; 4 x 8 likewise)
    ntt_checks(emu_library(), curve_id, G, EMU_TWO_PASS_LOGS, TWO_PASS)


@pytest.mark.parametrize("G", [2, 4, 8])
def test_emu_ntt_three_pass(G):
    assert ntt_plan(9, **THREE_PASS_3)["passes"] == 3 and shardable(9, 8, THREE_PASS_3) and not shardable(7, 8, THREE_PASS_3)
    ntt_checks(emu_library(), 0, G, EMU_THREE_PASS_LOGS, THREE_PASS_3)


@pytest.mark.parametrize("curve_id,G,logs,plan", [(0, 2, EMU_TWO_PASS_LOGS, TWO_PASS), (0, 4, EMU_TWO_PASS_LOGS, TWO_PASS), (1, 2, EMU_TWO_PASS_LOGS, TWO_PASS),
                                                  (1, 4, EMU_TWO_PASS_LOGS, TWO_PASS), (0, 2, EMU_THREE_PASS_LOGS, THREE_PASS_3),
                                                  (0, 4, EMU_THREE_PASS_LOGS, THREE_PASS_3), (0, 8, EMU_THREE_PASS_LOGS, THREE_PASS_3)],
                         ids=["bn254-2-two", "bn254-4-two", "bls12_381-2-two", "bls12_381-4-two", "bn254-2-three", "bn254-4-three", "bn254-8-three"])
def test_emu_witness_map(curve_id, G, logs, plan):
    witness_map_checks(emu_library(), curve_id, G, logs, plan)


@pytest.mark.parametrize("curve_id,G,rccl", [(0, 2, False), (0, 4, False), (0, 2, True), (2, 2, False)], ids=["bn254-2", "bn254-4", "bn254-2-gathered", "bls12_377-2"])
def test_emu_proof(curve_id, G, rccl):
    proof_checks(emu_library(), curve_id, G, 5, TWO_PASS, rccl=rccl)


def test_emu_proof_three_pass():
    proof_checks(emu_library(), 0, 2, 7, THREE_PASS_3)


def test_emu_fallbacks(monkeypatch):
    fallback_checks(emu_library(), 5, TWO_PASS, 5, (8, 5, TWO_PASS), monkeypatch)


def test_emu_a_failed_step_drops_every_member():
    """An assignment that is refused (z_0 != 1) fails in the first step on every member; a non-canonical entry is found when the
    tails collect, after three exchanges: both times nothing stays pending and the next proof is the right one."""
    case = proof_case(0, 5)
    multi = members(emu_library(), 2, TWO_PASS)
    try:
        load(multi, 0, case)
        multi.transform_shard(True)
        r, s = RS[0]
        for spoil in (lambda b: b.__setitem__(0, 2), lambda b: b.__setitem__(slice(64, 96), 0xff)):
            bad = np.array(case["z"], copy=True)
            spoil(bad)
            with pytest.raises(native.ZkhipError) as e:
                multi.prove_g16(bad, r, s)
            assert "member" in str(e.value)
            assert multi.prove_g16(case["z"], r, s) == case["want"](r, s) and multi.last_shard() == 2
            assert multi.ntt(0, ntt_reference(0, 5)[0], "fft").tobytes() == ntt_reference(0, 5)[1]["fft"] and multi.last_shard() == 2
    finally:
        multi.close()


# ================================================================== device
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = native.default_library()
    c = native.Context(0, L)
    assert "gfx950" in c.describe() and "EMULATOR" not in c.describe()
    c.close()
    return L


@gpu
@pytest.mark.parametrize("G", [2, 4, 8])
def test_gpu_ntt_default_plan(lib, G):
    assert [ntt_plan(n)["log1"] for n in (12, 13, 16)] == [6, 6, 8]          # two passes: 64 x 64, 64 x 128 (an odd split), 256 x 256
    ntt_checks(lib, 0, G, (12, 13, 16), {})


@gpu
def test_gpu_ntt_bls12_381(lib):
    ntt_checks(lib, 1, 4, (13,), {})


@gpu
def test_gpu_ntt_bls12_377(lib):
    multi = members(lib, 4, {})
    try:
        check_structured(multi, ref.CURVE, 13)          # (Multi.ntt has Context.ntt's signature)
        assert multi.last_shard() == 4
    finally:
        multi.close()


@gpu
@pytest.mark.parametrize("G", [2, 8])
def test_gpu_ntt_three_pass(lib, G):
    assert all(ntt_plan(n, **THREE_PASS_4)["passes"] == 3 for n in (9, 10, 11, 12))
    ntt_checks(lib, 0, G, (9, 10, 11, 12), THREE_PASS_4)


@gpu
@pytest.mark.parametrize("logn,G,plan", [(3, 2, TWO_PASS), (5, 4, TWO_PASS), (9, 8, THREE_PASS_3)], ids=["2x4-G2", "4x8-G4", "8x8x8-G8"])
def test_gpu_ntt_whole_and_sharded_where_the_tile_binds(lib, logn, G, plan):
    """One set of pass launchers runs the whole domain (zkhip_ntt on one context) and the strips and ranges of G members
    (zkhip_multi_ntt): both against cpu.ntt, byte for byte, in all four directions, at the plans where a strip is narrower than the
    plan's cols tile and a range has fewer rows than its rows tile — 2 x 4 over 2 members (G = N1 = Nb / 2: one row per range, two
    columns per strip), 4 x 8 over 4, and 8 x 8 x 8 over 8.  A launcher that gave a strip the whole plan's tile would run off its end."""
    p = ntt_plan(logn, **plan)
    N1, Nb = 1 << p["log1"], 1 << (p["log2"] + p["log3"])
    assert shardable(logn, G, plan) and p["passes"] == (3 if plan is THREE_PASS_3 else 2)
    assert Nb // G < p["C_cols"] and (N1 // G) * Nb >> (p["log3"] or p["log2"]) < p["R_rows"]          # both tiles bind
    a, want = ntt_reference(0, logn)
    multi = members(lib, G, plan)
    try:
        ctx = multi.member_context(0)
        for d in DIRS:
            assert ctx.ntt(0, a, d).tobytes() == want[d], ("whole", logn, d)
            assert multi.ntt(0, a, d).tobytes() == want[d], ("sharded", G, logn, d)
            assert multi.last_shard() == G
    finally:
        multi.close()


@gpu
def test_gpu_ntt_2e20_eight_members(lib):
    ntt_against_member0(lib, 0, 8, 20, DIRS)


@gpu
def test_gpu_ntt_2e23_natural_three_pass(lib):
    assert ntt_plan(23)["passes"] == 3
    ntt_against_member0(lib, 0, 8, 23, ("fft", "coset_ifft"))


@gpu
@pytest.mark.parametrize("G", [2, 4, 8])
def test_gpu_witness_map(lib, G):
    witness_map_checks(lib, 0, G, (12, 13), {}, kinds=("dense", "sha"))


@gpu
@pytest.mark.parametrize("logn", [12, 13])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_gpu_proof(lib, G, logn):
    proof_checks(lib, 0, G, logn, {})


@gpu
def test_gpu_proof_three_pass(lib):
    proof_checks(lib, 0, 4, 12, THREE_PASS_4)


@gpu
def test_gpu_proof_bls12_381(lib):
    proof_checks(lib, 1, 4, 12, {})


@gpu
def test_gpu_proof_every_gpu_a_member(lib):
    n = lib.device_count()
    if n < 2 or n & (n - 1):
        pytest.skip("needs a power-of-two number of GPUs >= 2 (this box has %d)" % n)
    proof_checks(lib, 0, n, 13, {}, devices=list(range(n)))
    proof_checks(lib, 0, n, 13, {}, devices=list(range(n)), rccl=True)


@gpu
def test_gpu_fallbacks(lib, monkeypatch):
    fallback_checks(lib, 12, {}, 10, (16, 9, THREE_PASS_4), monkeypatch)


@gpu
def test_gpu_same_bytes_under_stream_jitter(lib):
    """two proofs and two transforms with a spin kernel of random length ahead of half the enqueues (the knob of
    tests/test_stream_jitter.py): a missing ordering between a pack, a peer's copy and an unpack shows as other bytes"""
    case = proof_case(0, 13)
    a, want = ntt_reference(0, 13)
    multi = members(lib, 4, {})
    ctx = multi.member_context(0)
    try:
        load(multi, 0, case)
        multi.transform_shard(True)
        calm = [multi.prove_g16(case["z"], r, s) for r, s in RS] + [multi.ntt(0, a, d).tobytes() for d in ("fft", "coset_ifft")]
        assert calm == [case["want"](r, s) for r, s in RS] + [want["fft"], want["coset_ifft"]]
        ctx.tune("stream_jitter", 300)          # process-wide
        try:
            for rep in range(2):
                got = [multi.prove_g16(case["z"], r, s) for r, s in RS]
                assert multi.last_shard() == 4
                got += [multi.ntt(0, a, d).tobytes() for d in ("fft", "coset_ifft")]
                assert got == calm, rep
        finally:
            ctx.tune("stream_jitter", 0)
    finally:
        multi.close()
