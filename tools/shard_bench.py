#!/usr/bin/env python3
"""One proof over 8 members with the witness map replicated (today's path for an unbound key) against the same proof with the
transform domain sharded across the members (zkhip_multi_transform_shard), in ONE process: the dense synthetic circuit on bn128,
Groth16, the key NOT bound.

    python tools/shard_bench.py [--logs 20 22] [--members 8] [--steps 9] [--out profiles/transform_shard.json]

The members are dealt round-robin over the GPUs of the box.  ON ONE GPU THEY SHARE IT: they time-slice, every "peer copy" is a copy
inside one device's memory and the exchange is extra work on the device that also runs the transforms — the figure this writes is a
BASELINE for the first run on a node with more than one GPU, not a result, and no speed-up is claimed from it.  Switch off / on
ALTERNATE proof by proof, so that whatever else the box is doing falls on both; medians of the zkhip_timings the call returns
(the slowest member per phase; total = wall clock of the call).  Every proof is compared with the first one's bytes."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zokrates_amd import native, synth   # noqa: E402


def one_size(lib, lg, members, steps):
    ndev = lib.device_count()
    multi = native.Multi([k % ndev for k in range(members)], lib)
    try:
        circ = synth.circuit(0, lg, kind="dense")
        z = circ.assignment(0x5EED0000 + lg)
        ctx = multi.member_context(0)
        cs = native.ConstraintSystem(ctx, 0, circ.n, circ.l, circ.w, circ.mats())
        raw = native.setup_g16(ctx, cs, synth.toxic_waste(0))
        cs.close()
        multi.load_constraint_system(0, circ.n, circ.l, circ.w, circ.mats())
        multi.load_proving_key(0, raw)
        r, s = 0x123456789abcdef0123, 0xfedcba9876543210fed
        first = multi.prove_g16(z, r, s)             # (warm-up: plans, streams, buffers)
        multi.transform_shard(True)
        assert multi.prove_g16(z, r, s) == first and multi.last_shard() == members, "the sharded proof differs, or did not shard"
        runs = {"replicated": [], "sharded": []}
        for i in range(2 * steps):
            on = bool(i & 1)
            multi.transform_shard(on)
            proof, tm = multi.prove_g16(z, r, s, want_timings=True)
            assert proof == first and multi.last_shard() == (members if on else 0)
            runs["sharded" if on else "replicated"].append(tm)
        N = 1 << lg
        out = {"log_domain": lg, "members": members, "gpus": ndev, "steps": steps,
               # three all-to-alls of 3, 2 and 1 vectors: a member sends (and receives) (G - 1) / G of N / G elements of each
               "bytes_sent_per_member_per_proof": 6 * (N // members) * 32 * (members - 1) // members,
               "bytes_exchanged_per_proof": 6 * N * 32 * (members - 1) // members}
        for name, tms in runs.items():
            out[name] = {k: round(statistics.median(t[k] for t in tms), 3) for k in ("total_ms", "ntt_ms", "matvec_ms", "msm_h_ms", "msm_z_ms", "kernel_ntt_ms")}
        return out
    finally:
        multi.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_shard.json"))
    a = ap.parse_args()
    lib = native.default_library()
    ctx = native.Context(0, lib)
    desc = ctx.describe()
    ctx.close()
    doc = {"what": "zkhip_prove_g16_multi, unbound dense bn128 circuit, witness map replicated vs domain sharded (tools/shard_bench.py)",
           "caveat": "members share the GPU(s) of one box: a one-box BASELINE for the first multi-GPU run, not a result; no speed-up is claimed",
           "device": desc, "sizes": [one_size(lib, lg, a.members, a.steps) for lg in a.logs]}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
