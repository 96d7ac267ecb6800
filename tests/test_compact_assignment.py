"""Compact assignments: the "ZKHIPZ1" packed form of an assignment (include/zkhip.h), the host packer / unpacker, the upload that
widens it on the device (`zkhip_assignment_upload_packed`, `k_unpack_assignment`), the witness reader that emits it and
`generate-proof --compact-witness`.

The reference of every assertion is the encoder / decoder of the format written out in this file from the header's text (`encode`,
`decode`) and plain integers — never the library.  No tolerances: bytes and verdicts are compared for equality.

What a resident assignment holds is observed through `zkhip_r1cs_check` over a system with one row per variable — row k - 1 is
z_k * ONE = (the expected value) * ONE — so a wrong element is named by its row.

Every case that touches a device runs on the emulator (`-m "not gpu"`: bn128 and bls12_381) and on the GPU (`-m gpu`: bls12_377 as
well); malformed buffers go to the emulator only."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import ir
from oracle.fields import BN254, BLS12_381
from zokrates_amd import native, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NONE = (None, 0)
GPU = pytest.mark.gpu
BAD_ARG, PARSE, UNSATISFIED = -1, -2, -5
R_MAX = synth.FR_MODULUS[1]            # the largest scalar field of the supported curves (BLS12-381): what the curve-less packer refuses from
M_LIST = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2049, 4099)
WIDTH = (0, 1, 8, 32)


def on(backend, *values):
    return pytest.param(backend, *values, marks=[GPU] if backend == "gpu" else [], id="-".join([backend] + [str(v) for v in values]))


DEVICES = [on("emu", 0), on("emu", 1), on("gpu", 0), on("gpu", 1), on("gpu", 2)]
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


@pytest.fixture(scope="module")
def lib():
    from emu_util import emu_library
    return emu_library()


# ------------------------------------------------------------------ the format, from the header's text
def r16(x):
    return (x + 15) // 16 * 16


def minimal_class(v):
    return 0 if v == 0 else 1 if v < 256 else 2 if v < 1 << 64 else 3


def encode(values, classes=None):
    """The packed form of a list of integers below 2^256; `classes`: a class per element (default: the minimal one)."""
    m = len(values)
    classes = [minimal_class(v) for v in values] if classes is None else classes
    tags = bytearray(r16((m + 3) // 4))
    for i, c in enumerate(classes):
        tags[i // 4] |= c << (2 * (i % 4))
    nblocks = (m + 1023) // 1024
    index, payload = [0], bytearray()
    for b in range(nblocks):
        for i in range(1024 * b, min(m, 1024 * (b + 1))):
            assert values[i] < 1 << (8 * WIDTH[classes[i]]) or values[i] == 0
            payload += values[i].to_bytes(32, "little")[:WIDTH[classes[i]]]
        payload += bytes(r16(len(payload)) - len(payload))
        index.append(len(payload))
    if len(index) % 2:
        index.append(0)
    out = b"ZKHIPZ1\0" + m.to_bytes(8, "little") + len(payload).to_bytes(8, "little") + (1024).to_bytes(4, "little") + (0).to_bytes(4, "little")
    out += bytes(tags) + b"".join(x.to_bytes(8, "little") for x in index) + bytes(payload)
    return np.frombuffer(out, dtype=np.uint8)


class Malformed(Exception):
    pass


def decode(buf):
    """The list of integers of a packed buffer; Malformed (naming the rule) for one the format does not allow."""
    b = bytes(buf)

    def need(ok, what):
        if not ok:
            raise Malformed(what)

    need(len(b) >= 32, "header")
    need(b[:8] == b"ZKHIPZ1\0", "magic")
    u = lambda off, n: int.from_bytes(b[off:off + n], "little")
    m, payload_bytes, block, flags = u(8, 8), u(16, 8), u(24, 4), u(28, 4)
    need(block == 1024, "block")
    need(flags == 0, "flags")
    need(m <= 4 * len(b) and payload_bytes <= len(b), "length")
    ntag, nblocks = (m + 3) // 4, (m + 1023) // 1024
    tags_off = 32
    index_off = tags_off + r16(ntag)
    entries = nblocks + 1 + (nblocks + 1) % 2
    payload_off = index_off + 8 * entries
    need(len(b) == payload_off + payload_bytes, "length")
    need(payload_bytes % 16 == 0, "payload_bytes alignment")
    index = [u(index_off + 8 * k, 8) for k in range(entries)]
    need(index[0] == 0 and index[nblocks] == payload_bytes, "index ends")
    need(all(x == 0 for x in index[nblocks + 1:]), "index padding")
    tags = b[tags_off:index_off]
    cls = lambda i: (tags[i // 4] >> (2 * (i % 4))) & 3
    need(all(x % 16 == 0 for x in index), "index alignment")
    values = []
    for k in range(nblocks):
        need(index[k + 1] >= index[k], "index monotone")
        lo, hi = 1024 * k, min(m, 1024 * (k + 1))
        need(index[k + 1] - index[k] == r16(sum(WIDTH[cls(i)] for i in range(lo, hi))), "index span")
        p = payload_off + index[k]
        for i in range(lo, hi):
            w = WIDTH[cls(i)]
            values.append(int.from_bytes(b[p:p + w], "little"))
            p += w
    need(all(cls(i) == 0 for i in range(m, 4 * len(tags))), "tag padding")
    return values


def to_bytes(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint8)


def to_ints(z):
    z = bytes(z)
    return [int.from_bytes(z[i:i + 32], "little") for i in range(0, len(z), 32)]


def drawn(m, r, seed):
    """m values from {0, 1, 255, 256, 2^64 - 1, 2^64, r - 1} and random ones of every width; element 0 is 1."""
    rnd = random.Random(seed)
    special = [0, 1, 255, 256, (1 << 64) - 1, 1 << 64, r - 1]
    pick = lambda: rnd.choice(special) if rnd.random() < 0.6 else rnd.choice([rnd.randrange(256), rnd.randrange(1 << 64), rnd.randrange(r)])
    return [1] + [pick() for _ in range(m - 1)]


# ------------------------------------------------------------------ 1. the packer's bytes
@pytest.mark.parametrize("curve_id", [0, 1, 2])
def test_packer_bytes(lib, curve_id):
    r = synth.FR_MODULUS[curve_id]
    for m in M_LIST:
        values = drawn(m, r, 0xAC0 + 31 * m + curve_id)
        z = to_bytes(values)
        want = encode(values)
        got = native.pack_assignment(z, lib)
        assert got.tobytes() == want.tobytes(), m
        assert decode(got) == values
        assert native.unpack_assignment(got, lib).tobytes() == z.tobytes(), m
        # a wider class than needed decodes to the same value
        wide = encode(values, [min(3, minimal_class(v) + 1) for v in values])
        assert native.unpack_assignment(wide, lib).tobytes() == z.tobytes(), m
        # the bound holds the all-wide case
        allwide = encode([1] + [r - 1] * (m - 1), [3] * m)
        assert native.pack_bound(m, lib) >= allwide.size >= 32 * m
        assert native.pack_assignment(to_bytes([1] + [r - 1] * (m - 1)), lib).size <= native.pack_bound(m, lib)
        # one byte short: refused, and nothing written — the bytes before the end included
        out = np.full(want.size + 64, 0xA5, dtype=np.uint8)
        need = native.C.c_uint64()
        rc = lib.L.zkhip_assignment_pack(native._ptr(z), m, native._ptr(out), want.size - 1, native.C.byref(need))
        assert rc == BAD_ARG and need.value == want.size and (out == 0xA5).all(), m
        rc = lib.L.zkhip_assignment_pack(native._ptr(z), m, native._ptr(out), want.size, native.C.byref(need))
        assert rc == 0 and out[:want.size].tobytes() == want.tobytes() and (out[want.size:] == 0xA5).all(), m


def test_packer_refuses_what_no_field_holds(lib):
    """The packer has no curve: it refuses a value that is canonical in no supported field — r of BLS12-381, the largest, and 2^256 - 1.
    It is therefore NO canonicality gate for bn128 or bls12_377: their r (and anything up to BLS12-381's) packs, and is refused where
    the curve is known — by the upload, on the device (test_canonical_check), and by `Program.assignment_packed` on the host."""
    for m, k in ((1, 0), (5, 3), (1025, 1024), (2049, 1023)):
        for bad in (R_MAX, (1 << 256) - 1):
            values = drawn(m, R_MAX, 7)
            values[k] = bad
            with pytest.raises(native.ZkhipError) as e:
                native.pack_assignment(to_bytes(values), lib)
            assert e.value.code == BAD_ARG and f"entry {k} " in str(e.value)
        values[k] = R_MAX - 1
        assert decode(native.pack_assignment(to_bytes(values), lib)) == values


def test_packer_under_sanitizers(tmp_path):
    """tests/host/compact_pack.cpp under ASan + UBSan, a stand-alone program: the packer, the validation and the unpacker over heap
    blocks of exactly their sizes — packings at the block-boundary sizes, a cap one byte short, every prefix, 4 000 mutations."""
    exe = str(tmp_path / "compact_pack")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_EMU", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "zokrates_amd", "csrc"), "-x", "c++", os.path.join(HERE, "host", "compact_pack.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ 2. the expansion on the device
class OneRowPerVariable:
    """l = 1; row k - 1: z_k * ONE = values[k] * ONE.  An assignment that differs from `values` at k fails exactly row k - 1."""

    def __init__(self, ctx, curve_id, values):
        self.values, self.m, n = values, len(values), len(values) - 1
        rp = np.arange(n + 1, dtype=np.uint64)
        one = to_bytes([1] * n) if n else np.zeros(0, dtype=np.uint8)
        a = (rp, np.arange(1, n + 1, dtype=np.uint32), one)
        b = (rp, np.zeros(n, dtype=np.uint32), one)
        c = (rp, np.zeros(n, dtype=np.uint32), to_bytes(values[1:]) if n else np.zeros(0, dtype=np.uint8))
        self.cs = native.ConstraintSystem(ctx, curve_id, n, 1, n, [a, b, c])

    def verdict(self, ctx, values):
        """Of the packed upload of `values` (packed by the encoder above), held against the plain upload's and the host call's."""
        packed = encode(values)
        a = native.Assignment.from_packed(ctx, self.cs, packed)
        got = self.cs.check(a)
        a.close()
        zb = to_bytes(values)
        plain = native.Assignment(ctx, self.cs, zb)
        assert got == self.cs.check(plain) == self.cs.check(zb)
        plain.close()
        return got


def another(v, r):
    """A value next to v, mostly of another width: 0 -> 1 -> ... 255 -> 256, 2^64 - 1 -> 2^64, r - 1 -> 0."""
    return (v + 1) % r


def shapes(r):
    """name -> (values, positions whose corruption is tried)."""
    rnd = random.Random(0x5AFE)
    wide = lambda: rnd.randrange(1 << 200, r)
    out = {}
    for m in M_LIST:
        out[f"m{m}"] = (drawn(m, r, 0xD0 + m), {1, 2, 3, 4, 255, 256, 1023, 1024, 1025, 2047, 2048, m - 2, m - 1})
    # all-zero blocks between full ones: spans of length 0
    v = [1] + [wide() for _ in range(1023)] + [0] * 2048 + [wide() for _ in range(1024)] + [0] * 1024 + [7, 0, 0, 0, wide()]
    out["zero_blocks"] = (v, {1, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, 5119, 5120, 5124})
    # a block of 1024 values of 32 bytes: the 32 KiB span
    v = [1] + [0] * 1023 + [wide() for _ in range(1024)] + [3]
    out["full_span"] = (v, {1024, 1025, 1279, 1280, 1535, 1536, 2046, 2047, 2048})
    # classes cycling 0,1,2,3 and 3,2,1,0: values start at every offset mod 16
    by_class = lambda c: [0, rnd.randrange(1, 256), rnd.randrange(256, 1 << 64), wide()][c]
    out["cycle_up"] = ([1] + [by_class(i % 4) for i in range(1, 2100)], {1, 2, 3, 4, 5, 6, 7, 1024, 1027, 2099})
    out["cycle_down"] = ([1] + [by_class(3 - i % 4) for i in range(1, 2100)], {1, 2, 3, 4, 5, 6, 7, 1023, 1026, 2099})
    # a last block of 1, 3 and 1023 live elements (1 is also m1025 above)
    out["tail3"] = (drawn(1027, r, 0xE3), {1023, 1024, 1025, 1026})
    out["tail1023"] = (drawn(2047, r, 0xE4), {1024, 2044, 2045, 2046})
    # a 32-byte value at the first and last position of a block, of a wave (elements 255 | 256 of a block) and of a work-item, zeros around
    at = [1024, 2047, 1024 + 255, 1024 + 256, 1024 + 508, 1024 + 511, 2048, 3071, 3072 + 63 * 4 + 3, 3072 + 64 * 4]
    v = [1] + [0] * 4099
    for k in at:
        v[k] = wide()
    out["edges"] = (v, set(at) | {1023, 1025, 2046, 4099})
    return out


@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_device_expansion(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = synth.FR_MODULUS[curve_id]
    for name, (values, positions) in shapes(r).items():
        m = len(values)
        assert decode(encode(values)) == values
        system = OneRowPerVariable(ctx, curve_id, values)
        assert system.verdict(ctx, values) == NONE, name
        for k in sorted(p for p in positions if 1 <= p < m):
            changed = list(values)
            changed[k] = another(values[k], r)
            assert system.verdict(ctx, changed) == (k - 1, 1), (name, k)
        system.cs.close()


@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_wider_classes_and_argument_checks(contexts, backend, curve_id):
    """A non-minimal class decodes to the same value on the device; m != l + w and element 0 != 1 are ZKHIP_ERR_BAD_ARG with the plain
    upload's message for the latter."""
    ctx = context(contexts, backend)
    r = synth.FR_MODULUS[curve_id]
    values = drawn(1030, r, 0xF00D)
    system = OneRowPerVariable(ctx, curve_id, values)
    for bump in (1, 2, 3):
        a = native.Assignment.from_packed(ctx, system.cs, encode(values, [min(3, minimal_class(v) + bump) for v in values]))
        assert system.cs.check(a) == NONE
        a.close()
    for other in (values[:-1], values + [0]):
        with pytest.raises(native.ZkhipError) as e:
            native.Assignment.from_packed(ctx, system.cs, encode(other))
        assert e.value.code == BAD_ARG and "l + w" in str(e.value)
    with pytest.raises(native.ZkhipError) as plain:
        native.Assignment(ctx, system.cs, to_bytes([2] + values[1:]))
    for first, classes in ((2, None), (0, None), (257, None), (1 << 70, None), (0, [3] + [minimal_class(v) for v in values[1:]])):
        with pytest.raises(native.ZkhipError) as e:
            native.Assignment.from_packed(ctx, system.cs, encode([first] + values[1:], classes))
        assert e.value.code == BAD_ARG and str(e.value) == str(plain.value)
    a = native.Assignment.from_packed(ctx, system.cs, encode(values, [3] + [minimal_class(v) for v in values[1:]]))      # ONE, 32 bytes wide
    assert system.cs.check(a) == NONE
    a.close()
    system.cs.close()


# ------------------------------------------------------------------ 3. the canonical check
@pytest.mark.parametrize("backend,curve_id", DEVICES)
def test_canonical_check(contexts, backend, curve_id):
    ctx = context(contexts, backend)
    r = synth.FR_MODULUS[curve_id]
    values = drawn(2049, r, 0xCA70)
    system = OneRowPerVariable(ctx, curve_id, values)
    with pytest.raises(native.ZkhipError) as plain:
        native.Assignment(ctx, system.cs, to_bytes(values[:5] + [r] + values[6:]))
    assert plain.value.code == BAD_ARG and "canonical" in str(plain.value)
    for k in (1, 2048, 1023, 1024):
        for bad in (r, (1 << 256) - 1):
            with pytest.raises(native.ZkhipError) as e:
                native.Assignment.from_packed(ctx, system.cs, encode(values[:k] + [bad] + values[k + 1:]))
            assert e.value.code == BAD_ARG and str(e.value) == str(plain.value), (k, bad)
            # the context is usable afterwards
            assert system.verdict(ctx, values) == NONE
        ok = values[:k] + [r - 1] + values[k + 1:]
        assert system.verdict(ctx, ok) == (NONE if values[k] == r - 1 else (k - 1, 1))
    system.cs.close()


# ------------------------------------------------------------------ 4. the same proofs
def proving_case(ctx, curve_id, scheme):
    circ = synth.circuit(curve_id, log_domain=8)
    cs = native.ConstraintSystem(ctx, curve_id, circ.n, circ.l, circ.w, circ.mats())
    tox = synth.toxic_waste(curve_id)
    raw = native.setup_gm17(ctx, cs, (tox[0], tox[1], tox[2], tox[4])) if scheme == "gm17" else native.setup_g16(ctx, cs, tox)
    return circ, cs, native.ProvingKey(ctx, curve_id, raw, scheme=scheme)


PROOFS = [on("emu", "g16", 0), on("emu", "g16", 1), on("emu", "gm17", 0), on("emu", "gm17", 1), on("gpu", "g16", 0), on("gpu", "g16", 1), on("gpu", "g16", 2),
          on("gpu", "gm17", 0), on("gpu", "gm17", 1), on("gpu", "gm17", 2)]
RNDS = [(0x1111 * (i + 1), 0x2222 * (i + 3)) for i in range(3)]


@pytest.mark.parametrize("backend,scheme,curve_id", PROOFS)
def test_same_proofs(contexts, backend, scheme, curve_id):
    """The proof from the packed upload is the proof from the same z in host memory: a dense assignment (every element 32 bytes wide)
    and one of bits over the same system (checked mode off: satisfaction does not matter, the bytes do); one proof and a batch of 3."""
    ctx = context(contexts, backend)
    assert ctx.set_checked(None) is False
    circ, cs, pk = proving_case(ctx, curve_id, scheme)
    rnd = random.Random(0xB175)
    dense = circ.assignment(0x5EED)
    bits = to_bytes([1] + [rnd.randrange(2) for _ in range(cs.m - 1)])
    for z in (dense, bits):
        packed = native.pack_assignment(z, ctx.lib)
        assert packed.tobytes() == encode(to_ints(z)).tobytes()
        a = native.Assignment.from_packed(ctx, cs, packed)
        if scheme == "gm17":
            assert native.prove_gm17(ctx, pk, cs, a, RNDS[0][0], 7, RNDS[0][1]) == native.prove_gm17(ctx, pk, cs, z, RNDS[0][0], 7, RNDS[0][1])
            got = native.prove_gm17_resident_batch(ctx, pk, cs, [a] * 3, [(x, 7, y) for x, y in RNDS])[0]
            want = [native.prove_gm17(ctx, pk, cs, z, x, 7, y) for x, y in RNDS]
        else:
            assert native.prove_g16_resident(ctx, pk, cs, a, *RNDS[0]) == native.prove_g16(ctx, pk, cs, z, *RNDS[0])
            got = native.prove_g16_resident_batch(ctx, pk, cs, [a] * 3, RNDS)[0]
            want = native.prove_g16_batch(ctx, pk, cs, np.concatenate([z] * 3), RNDS)[0]
        assert got == want and len(set(got)) == 3
        a.close()
    assert (dense != bits).any() and native.pack_assignment(dense, ctx.lib).size >= dense.size > 16 * native.pack_assignment(bits, ctx.lib).size
    pk.close()
    cs.close()


@GPU
def test_gpu_sha256_proof_from_the_packed_witness():
    """One SHA-256 compression (m = 48 661, a witness of bits): packed 40 times smaller, the proof of the plain upload."""
    from zokrates_amd import sha256_circuit as sha
    ctx = native.Context(0)
    c = sha.circuit(0, 1)
    z = c.assignment(0x5EED)
    cs = native.ConstraintSystem(ctx, 0, c.n, c.l, c.w, c.mats())
    pk = native.ProvingKey(ctx, 0, native.setup_g16(ctx, cs, synth.toxic_waste(0)))
    packed = native.pack_assignment(z)
    assert packed.tobytes() == encode(to_ints(z)).tobytes() and 30 * packed.size < z.size
    a = native.Assignment.from_packed(ctx, cs, packed)
    assert cs.check(a) == NONE
    plain = native.Assignment(ctx, cs, z)
    want = native.prove_g16_resident(ctx, pk, cs, plain, 1234567, 7654321)
    assert native.prove_g16_resident(ctx, pk, cs, a, 1234567, 7654321) == want == native.prove_g16(ctx, pk, cs, z, 1234567, 7654321)
    pk.close()
    ctx.close()


# ------------------------------------------------------------------ 5. malformed buffers (emulator only: no out-of-bounds read may be provoked on a GPU)
def outcome(ctx, lib, system, buf, m_cap):
    """('refused', code) or ('accepted', values) of zkhip_assignment_unpack, and the same of the upload (its values: the verdict of the
    system built for `expect`)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    try:
        un = ("accepted", to_ints(native.unpack_assignment(buf, lib, m_cap=m_cap)))
    except native.ZkhipError as e:
        un = ("refused", e.code)
    try:
        a = native.Assignment.from_packed(ctx, system.cs, buf)
        up = ("accepted", system.cs.check(a))
        a.close()
    except native.ZkhipError as e:
        up = ("refused", e.code)
    return un, up


def test_malformed_buffers(lib):
    curve_id = 0
    r = synth.FR_MODULUS[curve_id]
    ctx = native.Context(0, lib)
    m = 2100
    values = drawn(m, r, 0xBAD)
    good = encode(values)
    assert native.pack_assignment(to_bytes(values), lib).tobytes() == good.tobytes()
    system = OneRowPerVariable(ctx, curve_id, values)
    assert outcome(ctx, lib, system, good, m) == (("accepted", values), ("accepted", NONE))
    ntag, tags_off = (m + 3) // 4, 32
    index_off = tags_off + r16(ntag)
    payload_off = index_off + 8 * 4
    u64 = lambda x: np.frombuffer(int(x).to_bytes(8, "little"), dtype=np.uint8)

    def patched(off, data):
        b = good.copy()
        b[off:off + len(data)] = data
        return b

    index = [int.from_bytes(good[index_off + 8 * k:index_off + 8 * k + 8].tobytes(), "little") for k in range(4)]
    assert index[0] == 0 < index[1] < index[2] < index[3] == good.size - payload_off
    last_tag = good.copy()      # element 2099 between 32 bytes and none: more than the rounding of its block's span can hide
    last_tag[tags_off + ntag - 1] = (good[tags_off + ntag - 1] & 0x3F) | (0 if good[tags_off + ntag - 1] >> 6 == 3 else 0xC0)
    directed = {
        "magic": patched(6, [ord("2")]),
        "block": patched(24, [0, 8, 0, 0]),
        "flags": patched(28, [1]),
        "one short": good[:-1],
        "one long": np.concatenate([good, np.zeros(1, dtype=np.uint8)]),
        "sixteen long": np.concatenate([good, np.zeros(16, dtype=np.uint8)]),
        "index not monotone": np.concatenate([good[:index_off + 8], u64(index[2]), u64(index[1]), good[index_off + 24:]]),
        "index entry unaligned": patched(index_off + 8, u64(index[1] + 8)),
        "index[0] not 0": patched(index_off, u64(16)),
        "index span against its tags": patched(index_off + 8, u64(index[1] + 16)),
        "last index entry": patched(payload_off - 8, u64(index[3] - 16)),
        "tag of the last element": last_tag,
        "padding tag": patched(tags_off + ntag, [1]),
        "payload_bytes": patched(16, u64(index[3] + 16)),
    }
    for name, buf in directed.items():
        un, up = outcome(ctx, lib, system, buf, m)
        assert un == ("refused", PARSE) and up == ("refused", PARSE), (name, un, up)
    # (2100 elements: four index entries.  An odd count gets a padding entry, which must be zero)
    odd = encode(drawn(1025, r, 5))
    odd_padding = odd.copy()
    odd_padding[32 + r16(257) + 24] = 16
    assert decode(odd) and native.unpack_assignment(odd, lib).size == 1025 * 32
    with pytest.raises(native.ZkhipError) as e:
        native.unpack_assignment(odd_padding, lib)
    assert e.value.code == PARSE and "padding" in str(e.value)
    # a header that names one element more: well-formed (its tag is 0) — the caller's m_cap and the system's l + w refuse it
    assert outcome(ctx, lib, system, patched(8, u64(m + 1)), m) == (("refused", BAD_ARG), ("refused", BAD_ARG))

    # seeded single-byte mutations.  What the reference decoder makes of the mutant decides what both entry points must do:
    #   not well-formed                       -> both ZKHIP_ERR_PARSE
    #   well-formed, another element count    -> the upload ZKHIP_ERR_BAD_ARG (l + w); unpack ZKHIP_ERR_BAD_ARG if it exceeds m_cap
    #   well-formed, the same m               -> unpack returns the decoder's values; the upload holds them too (the row of the one
    #                                            changed element fails, or none) unless they are no assignment of this curve — element
    #                                            0 not 1, a value >= r — which the upload refuses with ZKHIP_ERR_BAD_ARG
    # The payload is 98 % of this buffer's bytes and no rule reads it, so positions drawn over the whole buffer would leave the
    # rules all but untouched (6 of 300 refused): a quarter of the mutations goes to each section — header, tags, index, payload.
    sections = [(0, tags_off), (tags_off, index_off), (index_off, payload_off), (payload_off, good.size)]
    rnd = random.Random(0x300)
    accepted = refused = 0
    for trial in range(300):
        lo, hi = sections[trial % 4]
        at, flip = rnd.randrange(lo, hi), rnd.randrange(1, 256)
        buf = good.copy()
        buf[at] ^= flip
        un, up = outcome(ctx, lib, system, buf, m)
        try:
            dec = decode(buf)
        except Malformed:
            assert un == ("refused", PARSE) and up == ("refused", PARSE), (trial, at, un, up)
            refused += 1
            continue
        if len(dec) != m:      # (a byte of the header's m, and tags of zero where the count changed)
            assert 8 <= at < 16 and up == ("refused", BAD_ARG), (trial, at, up)
            assert un == (("refused", BAD_ARG) if len(dec) > m else ("accepted", dec)), (trial, at, un)
            refused += 1
            continue
        # (only a payload value byte, or a tag that keeps its block's span, can get here)
        assert at >= payload_off or tags_off <= at < tags_off + ntag, (trial, at)
        assert un == ("accepted", dec), (trial, at)
        diff = [k for k in range(m) if dec[k] != values[k]]
        if dec[0] != 1 or any(v >= r for v in dec):
            assert up == ("refused", BAD_ARG), (trial, at, up)
        else:
            assert up == ("accepted", (diff[0] - 1, len(diff)) if diff else NONE), (trial, at, up)
        accepted += 1
    assert accepted >= 1 and refused >= 100, (accepted, refused)
    system.cs.close()
    ctx.close()


# ------------------------------------------------------------------ 6. the program reader
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=lambda c: c.name)
def test_program_reader(lib, curve):
    from test_ingest import random_prog
    rnd = random.Random(77)
    for trial in range(12):
        prog = random_prog(curve, rnd, n=rnd.randrange(0, 40), n_args=rnd.randrange(0, 6), n_out=rnd.randrange(0, 4))
        p = native.Program(ir.serialize_prog(prog), lib)
        order = ir.ark_order(prog)[2]
        used = set(order) | {-(i + 1) for i in range(3)}
        for small in (False, True):      # field elements, then bits and bytes
            values = {v: (1 if v == 0 else rnd.randrange(256) if small and rnd.random() < 0.9 else rnd.randrange(curve.r)) for v in used}
            wit = ir.serialize_witness(values)
            z, inputs = p.assignment(wit)
            packed, inputs_p = p.assignment_packed(wit)
            assert packed.tobytes() == native.pack_assignment(z, lib).tobytes() == encode([1] + [values[v] for v in order[1:]]).tobytes()
            assert inputs_p.tobytes() == inputs.tobytes()
        missing = [v for v in order[1:]]
        if missing:
            wit = ir.serialize_witness({v: x for v, x in values.items() if v != missing[-1]})
            with pytest.raises(native.ZkhipError) as e:
                p.assignment_packed(wit)
            assert e.value.code == UNSATISFIED
        p.close()


# ------------------------------------------------------------------ 7. beside a pending split proof
@pytest.mark.parametrize("backend", [on("emu"), on("gpu")])
def test_pending_split_proof(contexts, backend):
    """A world of one shard: the key bound to its system, a proof pending between split_begin and split_end.  The packed upload is
    refused like every other upload, names the pending proof, and split_end yields the partial record it yields without the attempt."""
    from oracle import cpu
    from oracle import groth16 as g16
    ctx = context(contexts, backend)
    oc = cpu.Circuit.synth(0, 29, 0x5EED00F0)
    tox = cpu.toxic_bytes(g16.Toxic.from_seed(BN254))
    raw = cpu.ProvingKey.setup(oc, tox).serialize()
    z = oc.assignment()
    cs = native.ConstraintSystem(ctx, 0, oc.n, oc.l, oc.w, [oc.csr(q) for q in range(3)])
    pk = native.ProvingKey(ctx, 0, raw, rank=0, world=1)
    pk.bind_shard(cs, raw)
    packed = native.pack_assignment(z, ctx.lib)
    other = native.prove_g16_split_begin(ctx, pk, cs, z, 91, 92, 1)          # the half a partner would send
    native.prove_g16_split_abort(ctx)
    native.prove_g16_split_begin(ctx, pk, cs, z, 91, 92, 0)
    want = native.prove_g16_split_end(ctx, pk, cs, other)
    assert native.combine_g16(ctx, pk, [want], 91, 92) == cpu.trapdoor(oc, tox, z, 91, 92)
    native.prove_g16_split_begin(ctx, pk, cs, z, 91, 92, 0)
    for _ in range(2):
        with pytest.raises(native.ZkhipError) as e:
            native.Assignment.from_packed(ctx, cs, packed)
        assert e.value.code == BAD_ARG and "split proof is pending" in str(e.value)
    assert native.prove_g16_split_end(ctx, pk, cs, other).tobytes() == want.tobytes()
    a = native.Assignment.from_packed(ctx, cs, packed)                       # nothing pending any more
    assert cs.check(a) == NONE
    # ... and a packed resident assignment starts a split proof like any other
    native.prove_g16_split_begin(ctx, pk, cs, a, 91, 92, 0)
    assert native.prove_g16_split_end(ctx, pk, cs, other).tobytes() == want.tobytes()
    assert native.prove_g16_partial(ctx, pk, cs, a, 91, 92).tobytes() == native.prove_g16_partial(ctx, pk, cs, z, 91, 92).tobytes()
    pk.close()
    cs.close()


# ------------------------------------------------------------------ 8. the command line
def cli_files(tmp_path, lib, bits):
    """bits: def main(private bool[40] b, field x) -> field: every b_k (b_k - 1) = 0, return x * sum b_k — a witness of bits.
    Else: def main(private field a, field b) -> (field, field) over field elements of eight bytes — dense for its six variables."""
    r = BN254.r
    if bits:
        nb = 40
        cons = [ir.Constraint([(k, 1)], [(k, 1), (0, r - 1)], []) for k in range(1, nb + 1)]
        cons.append(ir.Constraint([(k, 1) for k in range(1, nb + 1)], [(nb + 1, 1)], [(-1, 1)]))
        prog = ir.Prog(BN254, [ir.Parameter(k, True) for k in range(1, nb + 1)] + [ir.Parameter(nb + 1, False)], cons, return_count=1)
        b = [(k * 7 + 3) % 5 < 2 for k in range(nb)]
        values = {0: 1, nb + 1: 3, -1: 3 * sum(b)}
        values.update({k + 1: int(v) for k, v in enumerate(b)})
    else:
        prog = ir.Prog(BN254, [ir.Parameter(1, True), ir.Parameter(2, False)], [
            ir.Constraint([(1, 1)], [(2, 1)], [(3, 1)]),
            ir.Constraint([(0, 1)], [(3, 1)], [(-1, 1)]),
            ir.Constraint([(0, 1)], [(2, 1), (3, 1)], [(-2, 1)]),
        ], return_count=2)
        a, b = 1234567, 7654321
        values = {0: 1, 1: a, 2: b, 3: a * b, -1: a * b, -2: a * b + b}
    paths = {k: str(tmp_path / (k + ("" if bits else ".dense"))) for k in ("out", "witness", "proving.key", "proof.json")}
    open(paths["out"], "wb").write(ir.serialize_prog(prog))
    open(paths["witness"], "wb").write(ir.serialize_witness(values))
    ctx = native.Context(0, lib)
    p = native.Program(open(paths["out"], "rb").read(), lib)
    packed, _ = p.assignment_packed(np.fromfile(paths["witness"], dtype=np.uint8))
    assert (2 * packed.size < 32 * p.m) == bits
    native.setup_g16(ctx, p.constraint_system(ctx), synth.toxic_waste(0)).tofile(paths["proving.key"])
    ctx.close()
    return paths


def cli_checks(paths, commands, env, bits):
    for cmd in commands:
        run = lambda *more: subprocess.run(cmd + ["generate-proof", "-i", paths["out"], "-w", paths["witness"], "-p", paths["proving.key"], "-j",
                                                  paths["proof.json"], "--entropy", "e"] + list(more), capture_output=True, text=True, cwd=ROOT, env=env)
        r = run()
        assert r.returncode == 0 and "compact witness" not in r.stdout, r.stderr
        proof = open(paths["proof.json"]).read()
        assert json.loads(proof)["proof"]["a"]
        os.remove(paths["proof.json"])
        for more in ((), ("--check",)):
            r = run("--compact-witness", *more)
            assert r.returncode == 0 and ("compact witness: uploaded packed" if bits else "compact witness: dense, uploaded plain") in r.stdout, r.stderr + r.stdout
            assert open(paths["proof.json"]).read() == proof
            os.remove(paths["proof.json"])


def test_cli_compact_witness_on_emulator(tmp_path):
    from emu_util import EMU_LIB, emu_library
    exe = os.path.join(HERE, "_emu", "zkhip-cli-emu")
    for bits in (True, False):
        cli_checks(cli_files(tmp_path, emu_library(), bits), ([exe], [os.sys.executable, "-m", "zokrates_amd.cli"]), dict(os.environ, ZKHIP_LIBRARY=EMU_LIB), bits)


@GPU
def test_cli_compact_witness_on_gpu(tmp_path):
    exe = os.path.join(ROOT, "zokrates_amd", "zkhip-cli")
    cli_checks(cli_files(tmp_path, native.default_library(), True), ([exe],), dict(os.environ), True)


def test_cli_compact_witness_from_wtns_on_emulator(tmp_path, monkeypatch, capsys):
    """A `.r1cs` / `.wtns` pair holds the plain m x 32 B: with the flag the Python CLI packs it by the same rule — a witness of bits
    goes up packed, a dense one plain, `proof.json` as without the flag (the witnesses need not satisfy the system for that)."""
    from emu_util import emu_library
    from zokrates_amd import cli, formats
    monkeypatch.setattr(native, "_default", emu_library())
    circ = synth.circuit(0, 4, seed=0x600D)
    rnd = random.Random(4)
    r1, pkp, pj = tmp_path / "c.r1cs", tmp_path / "proving.key", tmp_path / "proof.json"
    r1.write_bytes(formats.write_r1cs(0, circ.m, 0, circ.l - 1, circ.w, circ.mats()))
    cli.main(["setup", "-i", str(r1), "-p", str(pkp), "-v", str(tmp_path / "verification.key"), "--entropy", "unit test"])
    for name, z, says in (("bits", to_bytes([1] + [rnd.randrange(2) for _ in range(circ.m - 1)]), "uploaded packed"),
                          ("dense", circ.assignment(99), "dense, uploaded plain")):
        wt = tmp_path / (name + ".wtns")
        wt.write_bytes(formats.write_wtns(0, z))
        common = ["generate-proof", "-i", str(r1), "-w", str(wt), "-p", str(pkp), "-j", str(pj), "--entropy", "abc"]
        cli.main(common)
        assert "compact witness" not in capsys.readouterr().out
        plain = pj.read_text()
        pj.unlink()
        cli.main(common + ["--compact-witness"])
        assert "compact witness: " + says in capsys.readouterr().out
        assert pj.read_text() == plain
