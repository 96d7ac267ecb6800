#!/usr/bin/env python3
"""Compact assignments against plain ones on one device, in ONE process: what packing a witness on the host and widening it on the
device (`zkhip_assignment_upload_packed`) gains over copying its m x 32 bytes (`zkhip_assignment_upload`), on the two witnesses
that bound the question — stdlib SHA-256 as `bench.py` shapes it (21 compressions side by side, m ~ 1.03 M, a witness of bits) and
the dense synthetic circuit at 2^20 (every element a field element), both bn128 / Groth16, the key bound to its system.

    python tools/compact_bench.py [--log-domain 20] [--calls 21] [--step-limit 240] [--out profiles/compact_assignment.json]

Per workload:
  (a) upload_ms                  zkhip_assignment_upload against zkhip_assignment_upload_packed (each call returns after the device
                                 is synchronised and the canonical verdict is read back: the allocation of the (m + 2) x 32 B
                                 device buffer is inside the clock on both sides, freeing the assignment is outside it)
  (b) lone_proof_from_host_ms    zkhip_prove_g16(z in host memory) against upload_packed + zkhip_prove_g16_resident (the packed
                                 side's assignment freed outside the clock)
  (c) host_ms                    zkhip_assignment_pack; zkhip_prog_assignment_packed against zkhip_prog_assignment (witness file -> z)
  (d) bytes                      packed and plain
The two sides of (a), (b) and of the readers in (c) ALTERNATE call by call, so whatever else the box is doing falls on both; each
figure is the median of `--calls` wall clocks (at least 20) after two warm-up calls of either side.  Every step runs under
`--step-limit` seconds: one that overruns ends the process with status 3 and nothing after it is started.  A run on the test
emulator (ZKHIP_LIBRARY) only rehearses the tool: its timings mean nothing and no file is written."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zokrates_amd import native, synth   # noqa: E402
from zokrates_amd import sha256_circuit as sha   # noqa: E402


class StepLimit:
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _late(self, *_):
        sys.stderr.write("compact_bench: step '%s' exceeded %d s: stopping\n" % (self.what, self.seconds))
        sys.stderr.flush()
        os._exit(3)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._late)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def alternate(calls, sides, after=None):
    """sides = {name: fn}; two warm-up rounds, then `calls` rounds of every side in turn.  `after(result)` runs outside the clock.
    {name: {"samples", "median"}}"""
    after = after or (lambda _: None)
    for _ in range(2):
        for fn in sides.values():
            after(fn())
    samples = {k: [] for k in sides}
    for _ in range(calls):
        for k, fn in sides.items():
            t, out = ms(fn)
            samples[k].append(t)
            after(out)
    return {k: {"median": statistics.median(v), "min": min(v), "samples": [round(x, 4) for x in v]} for k, v in samples.items()}


def workload(ctx, name, circ, z, calls, step):
    cid = 0
    m = circ.m
    rec = {"constraints": circ.n, "variables": m}
    with step(name + ": system, setup, key, bind"):
        cs = native.ConstraintSystem(ctx, cid, circ.n, circ.l, circ.w, circ.mats())
        pk = native.ProvingKey(ctx, cid, native.setup_g16(ctx, cs, synth.toxic_waste(cid)))
        pk.bind(cs)
        assert pk.is_bound(cs)
    with step(name + ": pack"):
        packed = native.pack_assignment(z)
        assert native.unpack_assignment(packed).tobytes() == z.tobytes()
        zi = z.reshape(-1, 32)
        wide = zi[:, 8:].any(axis=1)
        low = zi[:, :8].copy().view("<u8").reshape(-1)
        rec["bytes"] = {"plain": int(z.size), "packed": int(packed.size), "packed_over_plain": packed.size / z.size,
                        "takes_the_packed_path": bool(2 * packed.size < z.size), "rule": "2 x packed < 32 m (generate-proof --compact-witness)",
                        "elements": {"zero": int((~wide & (low == 0)).sum()), "one_byte": int((~wide & (low > 0) & (low < 256)).sum()),
                                     "eight_bytes": int((~wide & (low >= 256)).sum()), "thirty_two_bytes": int(wide.sum())}}
    with step(name + ": same proof"):
        a = native.Assignment.from_packed(ctx, cs, packed)
        want = native.prove_g16(ctx, pk, cs, z, 11, 13)
        assert native.prove_g16_resident(ctx, pk, cs, a, 11, 13) == want, "the packed upload's proof differs"
        a.close()
    with step(name + ": (a) uploads"):
        rec["upload_ms"] = alternate(calls, {"plain": lambda: native.Assignment(ctx, cs, z),
                                             "packed": lambda: native.Assignment.from_packed(ctx, cs, packed)}, after=lambda a: a.close())
    with step(name + ": (b) lone proofs from host memory"):
        def via_packed():
            a = native.Assignment.from_packed(ctx, cs, packed)
            native.prove_g16_resident(ctx, pk, cs, a, 31, 37)
            return a
        rec["lone_proof_from_host_ms"] = alternate(calls, {"plain": lambda: native.prove_g16(ctx, pk, cs, z, 31, 37), "packed": via_packed},
                                                   after=lambda a: a.close() if isinstance(a, native.Assignment) else None)
    with step(name + ": (c) host side"):
        host = alternate(calls, {"zkhip_assignment_pack": lambda: native.pack_assignment(z)})
        ids = np.arange(m, dtype=np.int64)
        prog = native.Program(native.write_program(cid, circ.n, m, circ.mats(), ids=ids, args=[(j, False) for j in range(1, circ.l)]))
        wit = native.write_witness(ids, z)
        assert prog.m == m
        pz, _ = prog.assignment(wit)
        pp, _ = prog.assignment_packed(wit)
        assert pp.tobytes() == native.pack_assignment(pz).tobytes()
        host.update(alternate(calls, {"zkhip_prog_assignment": lambda: prog.assignment(wit), "zkhip_prog_assignment_packed": lambda: prog.assignment_packed(wit)}))
        prog.close()
        rec["host_ms"] = host
        rec["host_ms_note"] = "through the Python binding: each call also allocates and zero-fills its output arrays (m x 32 B plain, the bound packed)"
    pk.close()
    cs.close()
    up, lone = rec["upload_ms"], rec["lone_proof_from_host_ms"]
    print("%s: m %d, packed/plain %.4f | upload %.3f -> %.3f ms | lone proof from host %.3f -> %.3f ms | pack %.3f ms, reader %.3f -> %.3f ms" % (
        name, m, rec["bytes"]["packed_over_plain"], up["plain"]["median"], up["packed"]["median"], lone["plain"]["median"], lone["packed"]["median"],
        rec["host_ms"]["zkhip_assignment_pack"]["median"], rec["host_ms"]["zkhip_prog_assignment"]["median"],
        rec["host_ms"]["zkhip_prog_assignment_packed"]["median"]), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-domain", type=int, default=20)
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_assignment.json"))
    args = ap.parse_args()
    step = lambda what: StepLimit(args.step_limit, what)
    lg = args.log_domain
    ctx = native.Context(args.device)
    desc = ctx.describe()
    rehearsal = "EMULATOR" in desc
    if not rehearsal and args.calls < 20:
        sys.exit("at least 20 calls per region")
    doc = {"tool": "tools/compact_bench.py", "device": desc, "host": os.uname().nodename, "log_domain": lg, "calls_per_side": args.calls,
           "order": "the two sides of every comparison alternate call by call, one process; medians of wall clocks that end in a device synchronise",
           "scheme": "Groth16, bn128, key bound to its constraint system", "workloads": {}}
    with step("circuits"):
        per_hash = len(sha.template()[0])
        c_sha = sha.circuit(0, max(1, (1 << lg) // (per_hash + 7)))
        z_sha = c_sha.assignment(0x5EED)
        c_dense = synth.circuit(0, lg, kind="dense", seed=0xABCD + lg)
        z_dense = c_dense.assignment(0x5EED + lg)
    print("circuits: sha256_stdlib %d hashes, m %d; dense m %d" % (c_sha.hashes, c_sha.m, c_dense.m), flush=True)
    doc["workloads"]["sha256_stdlib"] = dict(workload(ctx, "sha256_stdlib", c_sha, z_sha, args.calls, step), hashes=c_sha.hashes)
    doc["workloads"]["dense"] = workload(ctx, "dense", c_dense, z_dense, args.calls, step)
    ctx.close()
    if rehearsal:
        print("rehearsal on the emulator: the timings mean nothing, nothing is written")
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
