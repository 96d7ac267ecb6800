"""The unsaturated field arithmetic as the DEVICE compiles it: zkhip_field_op fields 3 (Fq2), 4 (Fr) and 5 (Fq) — see
include/zkhip.h — against Python big integers, on all three curves.  One body: on the emulator build in the CPU suite, on the GPU
under `-m gpu`.

The kernels work on Montgomery images x R' mod p in B-bit limbs, so an operand is extreme when its IMAGE is: the canonical values
handed in are v = e / R' mod p for images e at 0, 1, p - 1, p - 2, every limb below the top one at 2^B - 1, single-limb patterns and
2^(B k) +- 1, crossed with each other, plus seeded random pairs.  tests/test_fieldu_contract.py holds the same operations to their
written bounds on the host; here the question is only whether the device computes the same integers."""
import random

import numpy as np
import pytest

import bls377_ref
from oracle.fields import BLS12_381, BN254
from zokrates_amd import native

from emu_util import emu_library

# (curve, curve id, limb width and count of Fr and of Fq, the non-residue of Fq2)
CURVES = [(BN254, 0, (29, 9), (29, 9), 1), (BLS12_381, 1, (29, 9), (28, 14), 1), (bls377_ref.CURVE, 2, (29, 9), (28, 14), 5)]
_ctx = {}


@pytest.fixture(scope="module")
def contexts():
    """backend name -> context, made on first use and closed when the module is done"""
    def get(backend):
        if backend not in _ctx:
            c = native.Context(0, emu_library()) if backend == "emu" else native.Context(0)
            d = c.describe()
            assert ("EMULATOR" in d) == (backend == "emu") and (backend == "emu" or "gfx950" in d), d
            _ctx[backend] = c
        return _ctx[backend]
    yield get
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def le(vals, nb):
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "little") for v in vals), dtype=np.uint8)


def images(p, B, N):
    """Montgomery images at the edges of the limb form (all < p)"""
    top = B * (N - 1)
    m = (1 << B) - 1
    e = {0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << top) - 1, ((p >> top) - 1) << top | ((1 << top) - 1), (p >> top) << top, (1 << (p.bit_length() - 1)) - 1}
    for k in range(N):
        e.update((m << (B * k), 1 << (B * k), (1 << (B * k)) - 1, (1 << (B * k)) + 1, ((1 << B) - 2) << (B * k)))
    return sorted(x % p for x in e if 0 <= x)


def operand_pairs(p, B, N, n_random, seed):
    Rinv = pow(1 << (B * N), -1, p)
    es = images(p, B, N)
    vs = [e * Rinv % p for e in es]
    rnd = random.Random(seed)
    a = [x for x in vs for _ in vs] + [rnd.randrange(p) for _ in range(n_random)]
    b = [y for _ in vs for y in vs] + [rnd.randrange(p) for _ in range(n_random)]
    return a, b


def single_field_ops(p):
    return [("add", lambda x, y: (x + y) % p), ("sub", lambda x, y: (x - y) % p), ("sub4", lambda x, y: (x - y) % p),
            ("mul", lambda x, y: x * y % p), ("sqr", lambda x, y: x * x % p), ("mul_loose", lambda x, y: x * y % p), ("sqr_loose", lambda x, y: x * x % p),
            ("relax8", lambda x, y: 8 * x % p), ("x3_numerator", lambda x, y: (x - 3 * y) % p),
            ("bf_sub4", lambda x, y: (x - y) * y % p), ("bf_sub8", lambda x, y: (3 * x - 7 * y) * x % p), ("bf_add", lambda x, y: (x + y) * x % p),
            ("mul_neg_lazy", lambda x, y: -x * y % p),
            ("mul_wide", lambda x, y: 12 * x * y % p), ("sqr_wide", lambda x, y: 9 * x * x % p), ("mulsub_wide", lambda x, y: (12 * x * y - 12 * x * x) % p)]


def fq2_ops(F2):
    q = F2.q
    k = lambda n, x: (n * x[0] % q, n * x[1] % q)
    sqr = lambda x, y: F2.mul(x, x)
    return [("add", F2.add), ("sub", F2.sub), ("mul", F2.mul), ("sqr", sqr), ("inv", lambda x, y: F2.inv(x) if x != (0, 0) else (0, 0)),
            ("mul_call", F2.mul), ("sqr_call", sqr), ("mulsub", lambda x, y: F2.sub(F2.mul(x, y), F2.mul(x, x))),
            ("mul_wide", lambda x, y: F2.mul(k(3, x), k(4, y))), ("sqr_wide", lambda x, y: F2.mul(k(3, x), k(3, x))),
            ("mulsub_wide", lambda x, y: F2.sub(F2.mul(k(3, x), k(4, y)), F2.mul(k(3, x), k(4, x))))]


@pytest.mark.parametrize("backend", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("field", [3, 4, 5])
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c[0].name)
def test_fieldu_device(contexts, curve, field, backend):
    C, cid, fr_form, fq_form, beta = curve
    ctx = contexts(backend)
    if field == 3:
        q, nb = C.q, C.fq_bytes
        B, N = fq_form
        F2 = bls377_ref.Fq2Beta(q, beta)
        # the full cross of the images and 2 000 random pairs, as for fields 4 and 5, in c0; c1 takes the same list rotated, so that
        # every image also stands in c1 and meets other images across the components
        a0, b0 = operand_pairs(q, B, N, 2000, "fq2/%d" % cid)
        a = list(zip(a0, a0[7:] + a0[:7]))
        b = list(zip(b0, b0[3:] + b0[:3]))
        assert len(a) >= 4000
        pack = lambda xs: le([v for x in xs for v in x], nb)
        for op, fn in fq2_ops(F2):
            got = ctx.field_op(cid, 3, op, pack(a), pack(b))
            want = pack([fn(x, y) for x, y in zip(a, b)])
            assert got.tobytes() == want.tobytes(), (C.name, field, op, _first_diff(got, want, 2 * nb, list(zip(a, b))))
        return
    p, nb, (B, N) = (C.r, 32, fr_form) if field == 4 else (C.q, C.fq_bytes, fq_form)
    a, b = operand_pairs(p, B, N, 2000, "f%d/%d" % (field, cid))
    assert len(a) >= 4000
    pa, pb = le(a, nb), le(b, nb)
    for op, fn in single_field_ops(p):
        got = ctx.field_op(cid, field, op, pa, pb)
        want = le([fn(x, y) for x, y in zip(a, b)], nb)
        assert got.tobytes() == want.tobytes(), (C.name, field, op, _first_diff(got, want, nb, list(zip(a, b))))


def _first_diff(got, want, nb, pairs):
    g, w = np.asarray(got).reshape(-1, nb), np.asarray(want).reshape(-1, nb)
    bad = np.nonzero((g != w).any(axis=1))[0]
    return "%d of %d differ; first: operands %r" % (len(bad), len(pairs), pairs[int(bad[0])]) if len(bad) else "sizes differ"


@pytest.mark.parametrize("backend", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_field_ids_above_five_are_refused(contexts, backend):
    ctx = contexts(backend)
    z = np.zeros(32, dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    call = lambda field, op: ctx.lib.L.zkhip_field_op(ctx.h, 0, field, op, 1, native._ptr(z), native._ptr(z), native._ptr(out))
    assert call(6, 0) != 0 and call(-1, 0) != 0 and call(4, 16) != 0 and call(5, 16) != 0 and call(3, 11) != 0
    assert call(4, 15) == 0 and call(5, 0) == 0
