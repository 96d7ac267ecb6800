"""Structured transform vectors, shared by tests/test_emu_kernels.py (emulator) and tests/test_gpu_parity.py (device).

Random vectors never make a butterfly compute a - a, (r - 1) + (r - 1) or a run of zeros: the cases where the lazy differences of
kernels_ntt.cuh sit at 0, at exactly K p, or at their maximum.  These vectors do, in every pass structure, and most of their
transforms have closed forms, which are asserted next to the oracle's answer (and stand in for it where the only oracle is the
Python radix-2 transform and the size would make it slow)."""
import numpy as np

from oracle import cpu
from oracle import groth16 as g16
from oracle.fields import inv

DIRS = ("fft", "ifft", "coset_fft", "coset_ifft")


def le(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8)


_vectors = {}


def vectors(curve, logn):
    """[(name, vector, {direction: closed form})] over the domain of 2^logn points (made once per curve and size)"""
    key = (curve.curve_id, logn)
    if key not in _vectors:
        _vectors[key] = _make_vectors(curve, logn)
    return _vectors[key]


def _powers(base, n, r):
    t, x = [], 1
    for _ in range(n):
        t.append(x)
        x = x * base % r
    return t


def _make_vectors(curve, logn):
    r, n = curve.r, 1 << logn
    dom = g16.Domain(curve, n)
    w, g = dom.omega, dom.g
    wi, gi, ni = inv(w, r), inv(g, r), inv(n, r)
    top = r - 1
    wt, wit, gt, git = _powers(w, n, r), _powers(wi, n, r), _powers(g, n, r), _powers(gi, n, r)       # w^i, w^-i, g^i, g^-i for i < n
    out = []

    def delta(v, k):
        return [v % r if i == k else 0 for i in range(n)]

    def constant(c):
        geo = (pow(g, n, r) - 1) % r          # sum_j (g w^i)^j = (g^n - 1) / (g w^i - 1)
        return {"fft": delta(n * c, 0), "ifft": delta(c, 0), "coset_ifft": delta(c, 0),
                "coset_fft": [c * geo * pow((g * wt[i] - 1) % r, -1, r) % r for i in range(n)]}

    def spike(v, k):
        return {"fft": [v * wt[i * k % n] % r for i in range(n)], "ifft": [ni * v * wit[i * k % n] % r for i in range(n)],
                "coset_fft": [v * gt[k] * wt[i * k % n] % r for i in range(n)], "coset_ifft": [ni * v * wit[i * k % n] * git[i] % r for i in range(n)]}

    out.append(("zeros", [0] * n, {d: [0] * n for d in DIRS}))
    out.append(("all r-1", [top] * n, constant(top)))
    out.append(("all 1", [1] * n, constant(1)))
    for k in sorted({0, n - 1, n // 2}):
        out.append(("r-1 at %d" % k, delta(top, k), spike(top, k)))
    alt = [top if i & 1 else 0 for i in range(n)]
    half = n // 2                            # odd positions: c w^i (n / 2) at i = 0 and i = n / 2, nothing elsewhere
    alt_fft = [0] * n
    alt_fft[0] = (alt_fft[0] + top * half) % r
    alt_fft[half % n] = (alt_fft[half % n] + top * half * wt[half % n]) % r
    alt_ifft = [0] * n
    alt_ifft[0] = (alt_ifft[0] + ni * top * half) % r
    alt_ifft[half % n] = (alt_ifft[half % n] + ni * top * half * wit[half % n]) % r
    out.append(("alternating 0, r-1", alt, {"fft": alt_fft, "ifft": alt_ifft} if n >= 2 else {}))
    out.append(("first half r-1", [top if i < half else 0 for i in range(n)], {}))
    for k in sorted({0, 1 % n, n - 1}):
        out.append(("w^(-%d i)" % k, [wit[k * i % n] for i in range(n)], {"fft": delta(n, k), "ifft": delta(1, (-k) % n)}))
    out.append(("(r-1) g^(-i)", [top * git[i] % r for i in range(n)], {"coset_fft": delta(n * top, 0)}))
    return out


_oracle = {}      # the reference is computed once per (curve, size, vector, direction) and shared by every configuration


def oracle_ntt(curve, logn, name, a, d, dom):
    key = (curve.curve_id, logn, name, d)
    if key not in _oracle:
        _oracle[key] = cpu.ntt(curve.curve_id, le(a), d).tobytes() if curve.curve_id in (0, 1) else le(getattr(dom, d)(a)).tobytes()
    return _oracle[key]


def check_structured(ctx, curve, logn, slow_oracle_max_log=10):
    """every vector through every direction on `ctx`.  The expected bytes are the oracle's, and equal to the closed form where there is
    one; for a curve whose only oracle is the Python transform, sizes above 2^slow_oracle_max_log use the closed form alone where it
    exists."""
    n = 1 << logn
    dom = g16.Domain(curve, n)
    fast = curve.curve_id in (0, 1)
    for name, a, closed in vectors(curve, logn):
        assert len(a) == n and all(0 <= x < curve.r for x in a)
        for d in DIRS:
            want = None
            if d in closed:
                want = le(closed[d]).tobytes()
            if fast or logn <= slow_oracle_max_log or want is None:
                orc = oracle_ntt(curve, logn, name, a, d, dom)
                assert want is None or orc == want, ("oracle against the closed form", curve.name, logn, name, d)
                want = orc
            got = ctx.ntt(curve.curve_id, le(a), d).tobytes()
            assert got == want, (curve.name, logn, name, d)
