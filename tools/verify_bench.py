#!/usr/bin/env python3
"""Verification on the device (zkhip_verify_g16_batch / zkhip_verify_gm17_batch), in ONE process on one device: verdicts per second
and milliseconds per call at several batch sizes.

    python tools/verify_bench.py [--repeats 5] [--step-limit 120] [--out profiles/device_verify.json]

Proofs come from the project's own prover over a tiny circuit (x_i * 1 = x_i per public input, two products of witness variables):
three distinct proofs per key, repeated to the batch's size — a verdict costs the same whatever the circuit, except for the l
scalar multiplications of the input combination.  Legs: bn128 Groth16 with l = 1 and l = 64 at batches 1, 20, 256 and 4096; one
line each for BLS12-381 Groth16 and bn128 GM17 (l = 1, batches 20 and 256).  A region is one call, host buffers in and verdicts
out, wall clock; the regions ALTERNATE over the legs within a repeat, and every figure is the median over the repeats.  Every
verdict of every region must be 1.  Every step runs under `--step-limit` seconds: a step that overruns ends the process with
status 3 and nothing after it is started.  Writes one JSON document.

The baseline is the host verifier on the SAME proofs on one thread: the first proof of every leg and its key, written as
`verification.key` / `proof.json`, through `zkhip-cli verify --timings --repeat 4` (csrc/host/verify.cpp; no GPU in that process) — one
such process per repeat, between the device regions; the figure is the median of the in-process times of the check alone, each
process's first (which derives the curve's constants) left out.  Its answer must be PASSED.

Not measured here: the prover's own proofs/s on the same box — `python bench.py`, run once next to this."""
import argparse
import json
import os
import random
import signal
import subprocess
import tempfile
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zokrates_amd import native, synth   # noqa: E402

FR = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
      1: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}


class StepLimit:
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _late(self, *_):
        sys.stderr.write("verify_bench: step '%s' exceeded %d s: stopping\n" % (self.what, self.seconds))
        sys.stderr.flush()
        os._exit(3)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._late)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def tiny_system(ctx, cid, n_pub):
    one = (1).to_bytes(32, "little")
    rows = [((i,), (0,), (i,)) for i in range(1, n_pub + 1)] + [((n_pub + 1,), (n_pub + 1,), (n_pub + 2,)), ((n_pub + 2,), (n_pub + 1,), (n_pub + 3,))]
    mats = []
    for k in range(3):
        cols = [r[k][0] for r in rows]
        mats.append((np.arange(len(rows) + 1, dtype=np.uint64), np.array(cols, dtype=np.uint32), np.frombuffer(one * len(cols), dtype=np.uint8)))
    return native.ConstraintSystem(ctx, cid, len(rows), n_pub + 1, 3, mats)


CURVE_NAMES = {0: "bn128", 1: "bls12_381"}
CLI = os.path.join(ROOT, "zokrates_amd", "zkhip-cli")


def host_files(d, tag, cid, scheme, raw, proof, inputs):
    """`verification.key` and `proof.json` for the key at the head of `raw` and one proof record: the files the host verifier reads"""
    fq = 32 if cid == 0 else 48
    raw = bytes(raw)
    hx = lambda b: "0x" + bytes(b)[::-1].hex()
    g1 = lambda b, o: [hx(b[o:o + fq]), hx(b[o + fq:o + 2 * fq])]
    g2 = lambda b, o: [[hx(b[o:o + fq]), hx(b[o + fq:o + 2 * fq])], [hx(b[o + 2 * fq:o + 3 * fq]), hx(b[o + 3 * fq:o + 4 * fq])]]
    vk = {"scheme": scheme, "curve": CURVE_NAMES[cid]}
    if scheme == "g16":
        vk.update(alpha=g1(raw, 0), beta=g2(raw, 2 * fq), gamma=g2(raw, 6 * fq), delta=g2(raw, 10 * fq))
        at, qname = 14 * fq, "gamma_abc"
    else:
        vk.update(h=g2(raw, 0), g_alpha=g1(raw, 4 * fq), h_beta=g2(raw, 6 * fq), g_gamma=g1(raw, 10 * fq), h_gamma=g2(raw, 12 * fq))
        at, qname = 16 * fq, "query"
    n = int.from_bytes(raw[at:at + 8], "little")
    vk[qname] = [g1(raw, at + 8 + 2 * fq * i) for i in range(n)]
    doc = {"scheme": scheme, "curve": CURVE_NAMES[cid], "proof": {"a": g1(proof, 0), "b": g2(proof, 2 * fq), "c": g1(proof, 6 * fq)},
           "inputs": [hx(inputs[32 * i:32 * i + 32]) for i in range(len(inputs) // 32)]}
    paths = os.path.join(d, tag + ".key"), os.path.join(d, tag + ".json")
    json.dump(vk, open(paths[0], "w"))
    json.dump(doc, open(paths[1], "w"))
    return paths


def host_verify_ms(paths):
    """one `zkhip-cli verify` process: the in-process times of the check alone (csrc/host/verify.cpp, one thread), the first left out"""
    r = subprocess.run([CLI, "verify", "-v", paths[0], "-j", paths[1], "--timings", "--repeat", "4"], capture_output=True, text=True, timeout=110)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and "PASSED" in lines, (r.stdout, r.stderr)
    return json.loads([ln for ln in lines if ln.startswith("timings ")][0][8:])["verify_ms"][1:]


def make_leg(ctx, cid, scheme, n_pub):
    """(verifying key, three proof records, their inputs as bytes, the proving key's bytes)"""
    cs = tiny_system(ctx, cid, n_pub)
    tox = synth.toxic_waste(cid)
    raw = native.setup_g16(ctx, cs, tox) if scheme == "g16" else native.setup_gm17(ctx, cs, (tox[0], tox[1], 1, tox[4]))
    pk = native.ProvingKey(ctx, cid, raw, scheme=scheme)
    rnd = random.Random(1000 * n_pub + cid)
    proofs, inputs = [], []
    for k in range(3):
        xs = [rnd.randrange(FR[cid]) for _ in range(n_pub)]
        w1 = rnd.randrange(1, FR[cid])
        z = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in [1] + xs + [w1, w1 * w1 % FR[cid], w1 * w1 % FR[cid] * w1 % FR[cid]]), dtype=np.uint8)
        proofs.append(native.prove_g16(ctx, pk, cs, z, 11 + k, 7 * k + 3) if scheme == "g16" else native.prove_gm17(ctx, pk, cs, z, 11 + k, 7 * k + 3, 5 * k + 2))
        inputs.append(b"".join(x.to_bytes(32, "little") for x in xs))
    vk = native.VerificationKey(ctx, cid, raw, scheme=scheme)
    pk.close()
    cs.close()
    return vk, proofs, inputs, raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_verify.json"))
    args = ap.parse_args()
    step = lambda what: StepLimit(args.step_limit, what)
    ctx = native.Context(args.device)
    doc = {"tool": "tools/verify_bench.py", "device": ctx.describe(), "repeats": args.repeats, "order": "one call per leg, legs alternating within a repeat; medians",
           "region": "one zkhip_verify_*_batch call: host buffers in, verdicts out, wall clock", "legs": []}
    legs, hosts = [], []
    tmp = tempfile.mkdtemp(prefix="verify_bench_")
    for name, cid, scheme, n_pub, batches in (("bn128 g16 l=1", 0, "g16", 1, (1, 20, 256, 4096)), ("bn128 g16 l=64", 0, "g16", 64, (1, 20, 256, 4096)),
                                              ("bls12_381 g16 l=1", 1, "g16", 1, (20, 256)), ("bn128 gm17 l=1", 0, "gm17", 1, (20, 256))):
        with step("prepare " + name):
            vk, proofs, inputs, raw = make_leg(ctx, cid, scheme, n_pub)
            hosts.append({"name": name, "paths": host_files(tmp, name.replace(" ", "_").replace("=", ""), cid, scheme, raw, proofs[0], inputs[0]), "ms": []})
        fn = native.verify_g16_batch if scheme == "g16" else native.verify_gm17_batch
        for b in batches:
            pr = np.frombuffer(b"".join(proofs[i % 3] for i in range(b)), dtype=np.uint8)
            ins = np.frombuffer(b"".join(inputs[i % 3] for i in range(b)), dtype=np.uint8)
            legs.append({"name": name, "batch": b, "fn": fn, "vk": vk, "proofs": pr, "inputs": ins, "ms": []})
    with step("warm-up"):
        for leg in legs:
            assert list(leg["fn"](ctx, leg["vk"], leg["proofs"], leg["inputs"])) == [1] * leg["batch"], leg["name"]
    for rep in range(args.repeats):
        for leg in legs:
            with step("%s batch %d repeat %d" % (leg["name"], leg["batch"], rep)):
                t0 = time.perf_counter()
                ok = leg["fn"](ctx, leg["vk"], leg["proofs"], leg["inputs"])
                leg["ms"].append(1e3 * (time.perf_counter() - t0))
                assert int(ok.sum()) == leg["batch"], leg["name"]
        for h in hosts:
            with step("host verifier, %s, repeat %d" % (h["name"], rep)):
                h["ms"] += host_verify_ms(h["paths"])
    for leg in legs:
        ms = statistics.median(leg["ms"])
        doc["legs"].append({"leg": leg["name"], "batch": leg["batch"], "ms_per_call": ms, "verdicts_per_s": 1e3 * leg["batch"] / ms, "samples_ms": leg["ms"]})
        print("%-20s batch %5d: %9.3f ms per call, %9.1f verdicts/s" % (leg["name"], leg["batch"], ms, 1e3 * leg["batch"] / ms), flush=True)
    doc["host_verifier"] = {"what": "zkhip-cli verify --timings --repeat 4 on the first proof of each leg, one process per repeat between the device regions: "
                                    "the check alone (csrc/host/verify.cpp), one thread, each process's first sample left out", "legs": []}
    for h in hosts:
        ms = statistics.median(h["ms"])
        doc["host_verifier"]["legs"].append({"leg": h["name"], "ms_per_proof": ms, "verdicts_per_s": 1e3 / ms, "samples_ms": h["ms"]})
        print("%-20s host verifier, one thread: %9.3f ms per proof, %9.1f verdicts/s" % (h["name"], ms, 1e3 / ms), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
