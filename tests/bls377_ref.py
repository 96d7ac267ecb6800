"""BLS12-377 reference for the tests of the third curve, built from the oracle's curve-agnostic parts.  TEST CODE ONLY.

The oracle's own group code fixes Fq2 = Fq[u]/(u^2 + 1) and its C++ half knows two curves; neither changes.  What is curve
agnostic there — `oracle.fields.Curve`, `oracle.curves.Group` over any field-ops object, the Fr arithmetic of
`oracle.groth16` / `oracle.gm17` (QAP / SAP at the trapdoor, witness maps, closed-form proof scalars), `oracle.formats` and
`oracle.pairing` — is used as it is; this module adds the constants, an Fq2 with u^2 = -5, and a context manager that hands
`groups(curve)` of the two scheme modules the BLS12-377 groups for the duration of a call.

Constants: [UPSTREAM] ark-bls12-377 0.3.0.  The generators are checked here to be on their curves and of order r; that ark uses
exactly these points is not checked (only a setup without explicit generators depends on it)."""
import contextlib

from oracle import curves as ocurves
from oracle import gm17 as ogm17
from oracle import groth16 as og16
from oracle.fields import Curve, FqOps, inv

R = 8444461749428370424248824938781546531375899335154063827935233455917409239041
Q = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
BETA = 5                    # Fq2 = Fq[u]/(u^2 + 5)
B2 = (0, 155198655607781456406391640216936120121836107652948796323930557600032281009004493664981332883744016074664192874906)   # 1 / u

CURVE = Curve(
    name="bls12_377", curve_id=2, r=R, q=Q,
    fr_generator=22, two_adicity=47,
    two_adic_root=0x11d4b7f60cb92cc160c69477d1a8a12f9b506ee363e3f04a476ef4a4ec2a895e,
    b1=1, b2=B2,
    g1=(0x008848defe740a67c8fc6225bf87ff5485951e2caa9d41bb188282c8bd37cb5cd5481512ffcd394eeab9b16eb21be9ef,
        0x01914a69c5102eff1f674f5d30afeec4bd7fb348ca3e52d96d182ad44fb82305c2fe3d3634a9591afd82de55559c8ea6),
    g2=((0x018480be71c785fec89630a2a3841d01c565f071203e50317ea501f557db6b9b71889f52bb53540274e3e48f7c005196,
         0x00ea6040e700403170dc5a51b1b140d5532777ee6651cecbe7223ece0799c9de5cf89984bff76fe6b26bfefa6ea16afe),
        (0x00690d665d446f7bd960736bcbb2efb4de03ed7274b49a58e458c282f832d204f2cf88886d8c7c2ef094094409fd4ddf,
         0x00f8169fd28355189e549da3151a70aa61ef11ac3d591bf12463b01acee304c24279b83f5e52270bd9a1cdd185eb8f93)),
    fq_bytes=48,
)
PROGRAM_FILE_ID = bytes.fromhex("c2955ab5")     # sha256(r as 32 little-endian bytes)[:4]


class Fq2Beta:
    """The interface of oracle.fields.Fq2Ops over Fq[u]/(u^2 + beta)."""

    def __init__(self, q, beta):
        self.q, self.beta, self.zero, self.one = q, beta, (0, 0), (1, 0)

    def add(self, a, b): return ((a[0] + b[0]) % self.q, (a[1] + b[1]) % self.q)
    def sub(self, a, b): return ((a[0] - b[0]) % self.q, (a[1] - b[1]) % self.q)
    def neg(self, a): return ((-a[0]) % self.q, (-a[1]) % self.q)
    def mul(self, a, b): return ((a[0] * b[0] - self.beta * a[1] * b[1]) % self.q, (a[0] * b[1] + a[1] * b[0]) % self.q)
    def is_zero(self, a): return a[0] % self.q == 0 and a[1] % self.q == 0
    def small(self, k): return (k % self.q, 0)

    def inv(self, a):
        n = inv((a[0] * a[0] + self.beta * a[1] * a[1]) % self.q, self.q)
        return (a[0] * n % self.q, (-a[1]) * n % self.q)


F2 = Fq2Beta(Q, BETA)


def groups377(curve=CURVE):
    assert curve.name == "bls12_377"
    return ocurves.Group(FqOps(Q), CURVE.b1, CURVE.g1), ocurves.Group(F2, CURVE.b2, CURVE.g2)


@contextlib.contextmanager
def oracle_groups():
    """oracle.groth16 / oracle.gm17 call `groups(curve)` by name: inside this block the name answers for BLS12-377 too."""
    def groups(curve):
        return groups377(curve) if curve.name == "bls12_377" else ocurves.groups(curve)
    saved = og16.groups, ogm17.groups
    og16.groups = ogm17.groups = groups
    try:
        yield
    finally:
        og16.groups, ogm17.groups = saved


def g16_setup(cs, tox):
    with oracle_groups():
        return og16.setup(CURVE, cs, tox)


def g16_prove(cs, pk, z, r_, s_):
    with oracle_groups():
        return og16.prove(CURVE, cs, pk, z, r_, s_)


def g16_trapdoor(cs, tox, z, r_, s_):
    G1, G2 = groups377()
    la, lb, lc = og16.trapdoor_scalars(CURVE, cs, tox, z, r_, s_)
    return G1.amul(G1.gen, la), G2.amul(G2.gen, lb), G1.amul(G1.gen, lc)


def gm17_setup(cs, tox):
    with oracle_groups():
        return ogm17.setup(CURVE, cs, tox)


def gm17_prove(cs, pk, z, d1, d2, r_):
    with oracle_groups():
        return ogm17.prove(CURVE, cs, pk, z, d1, d2, r_)


def gm17_trapdoor(cs, tox, z, d1, r_):
    G1, G2 = groups377()
    la, lb, lc = ogm17.trapdoor_scalars(CURVE, cs, tox, z, d1, r_)
    return G1.amul(G1.gen, la), G2.amul(G2.gen, lb), G1.amul(G1.gen, lc)


def csr(cs):
    """The three matrices of an oracle.groth16.R1CS as (rowptr u64, col u32, val u8[nnz * 32]) for native.ConstraintSystem."""
    import numpy as np
    out = []
    for M in (cs.A, cs.B, cs.C):
        rp, col, val = [0], [], []
        for row in M:
            for j, v in row:
                col.append(j)
                val.append(int(v % R).to_bytes(32, "little"))
            rp.append(len(col))
        out.append((np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), np.frombuffer(b"".join(val), dtype=np.uint8).copy()))
    return out
