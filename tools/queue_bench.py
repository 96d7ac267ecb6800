#!/usr/bin/env python3
"""The proof queue against the batch calls and against back-to-back single calls on one device, in ONE process: the dense synthetic
circuit on bn128, Groth16, the key bound to its constraint system, the stream plan and 16 hardware queues requested as `bench.py`
requests them.

    python tools/queue_bench.py [--log-domain 20] [--steps 20] [--repeats 3] [--step-limit 240] [--sha-hashes 0] [--out profiles/proof_queue.json]

Regions of `--steps` proofs each, ALTERNATING (a, b, c, d, e, a, b, ...) so that whatever else the box is doing falls on all of them:

  a  back-to-back zkhip_prove_g16_resident calls            (what a host that proves each witness as it arrives does today)
  b  one zkhip_prove_g16_resident_batch call                (the rate to reach)
  c  the queue in its steady state over the same resident assignments: submit until full, then one collect per submit
  d  one zkhip_prove_g16_batch call from host memory
  e  the queue fed from host memory (zkhip_queue_submit with z)
  f  (--sha-hashes N > 0) the stdlib SHA-256 circuit, N independent compressions: packed submits against zkhip_assignment_upload_packed followed
     by a single resident proof

For (c) and (e) the submit-to-collect-return latency of every proof is kept (median reported).  Every step runs under `--step-limit`
seconds: a step that overruns ends the process with status 3 and nothing after it is started.  Writes one JSON document; a caller
that alternated `bench.py` on the parent commit and on this tree passes the two result lines with --bench-parent / --bench-tree."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zokrates_amd import native, synth   # noqa: E402


class StepLimit:
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _late(self, *_):
        sys.stderr.write("queue_bench: step '%s' exceeded %d s: stopping\n" % (self.what, self.seconds))
        sys.stderr.flush()
        os._exit(3)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._late)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def queue_region(q, sources, rs, packed=False):
    """`len(rs)` proofs through the open queue in the steady state; (seconds, [submit-to-collect-return latency in ms], proofs)"""
    cap = q.state()[0]
    put, lat, proofs, flying = {}, [], [], 0
    t0 = time.perf_counter()
    for k, rnd in enumerate(rs):
        if flying == cap:
            t, proof = q.collect()
            lat.append(1e3 * (time.perf_counter() - put.pop(t)))
            proofs.append(proof)
            flying -= 1
        ts = time.perf_counter()
        t = q.submit_packed(sources[k], rnd) if packed else q.submit(sources[k], rnd)
        put[t] = ts
        flying += 1
    while flying:
        t, proof = q.collect()
        lat.append(1e3 * (time.perf_counter() - put.pop(t)))
        proofs.append(proof)
        flying -= 1
    return time.perf_counter() - t0, lat, proofs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-domain", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sha-hashes", type=int, default=0)
    ap.add_argument("--bench-parent", default=None, help="file with bench.py's result lines on the parent commit")
    ap.add_argument("--bench-tree", default=None, help="file with bench.py's result lines on this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proof_queue.json"))
    args = ap.parse_args()
    step = lambda what: StepLimit(args.step_limit, what)
    cid, lg, nw, steps = 0, args.log_domain, 4, args.steps
    native.default_library().init(16)
    ctx = native.Context(args.device)
    ctx.tune("pipe_plan", 1)
    doc = {"tool": "tools/queue_bench.py", "device": ctx.describe(), "workload": "synthetic R1CS dense, bn128, Groth16, key bound to its system",
           "log_domain": lg, "steps_per_region": steps, "regions_per_kind": args.repeats, "hw_queues_requested": 16, "pipe_plan": 1,
           "order": "regions alternate a, b, c, d, e", "regions": {}}
    with step("setup"):
        circ = synth.circuit(cid, lg, kind="dense", seed=0xABCD + lg)
        cs = native.ConstraintSystem(ctx, cid, circ.n, circ.l, circ.w, circ.mats())
        raw = native.setup_g16(ctx, cs, synth.toxic_waste(cid))
    with step("key load and bind"):
        pk = native.ProvingKey(ctx, cid, raw)
        del raw
        pk.bind(cs)
        assert pk.is_bound(cs)
        hz = [circ.assignment(0x5EED + lg + i) for i in range(nw)]
        zs = [native.Assignment(ctx, cs, z) for z in hz]
    doc["constraints"] = circ.n
    import numpy as np
    host_all = np.concatenate([hz[j % nw] for j in range(steps)])
    rs = lambda rep: [(1000 * rep + j + 1, 7 + j) for j in range(steps)]
    with step("warm-up"):
        want = [native.prove_g16_resident(ctx, pk, cs, zs[j % nw], *rs(0)[j]) for j in range(4)]
        assert native.prove_g16_resident_batch(ctx, pk, cs, [zs[j % nw] for j in range(4)], rs(0)[:4])[0] == want
        assert native.prove_g16_batch(ctx, pk, cs, host_all[:4 * circ.m * 32], rs(0)[:4])[0] == want
        with native.ProofQueue(ctx, pk, cs) as q:
            doc["queue_capacity"] = q.state()[0]
            assert queue_region(q, [zs[j % nw] for j in range(4)], rs(0)[:4])[2] == want, "the queue's proofs differ from the single calls'"
            assert queue_region(q, [hz[j % nw] for j in range(4)], rs(0)[:4])[2] == want
    kinds = ("a_resident_singles", "b_resident_batch", "c_queue_resident", "d_host_batch", "e_queue_host")
    reg = {k: {"region_proofs_per_s": []} for k in kinds}
    for k in ("c_queue_resident", "e_queue_host"):
        reg[k]["latency_ms"] = []
    for rep in range(args.repeats):
        r = rs(rep + 1)
        res = [zs[j % nw] for j in range(steps)]
        for kind in kinds:
            with step("region %d %s" % (rep, kind)):
                if kind == "a_resident_singles":
                    t0 = time.perf_counter()
                    for j in range(steps):
                        native.prove_g16_resident(ctx, pk, cs, res[j], *r[j])
                    dt = time.perf_counter() - t0
                elif kind == "b_resident_batch":
                    t0 = time.perf_counter()
                    native.prove_g16_resident_batch(ctx, pk, cs, res, r)
                    dt = time.perf_counter() - t0
                elif kind == "d_host_batch":
                    t0 = time.perf_counter()
                    native.prove_g16_batch(ctx, pk, cs, host_all, r)
                    dt = time.perf_counter() - t0
                else:
                    with native.ProofQueue(ctx, pk, cs) as q:
                        dt, lat, _ = queue_region(q, res if kind == "c_queue_resident" else [hz[j % nw] for j in range(steps)], r)
                    reg[kind]["latency_ms"] += lat
            reg[kind]["region_proofs_per_s"].append(steps / dt)
    for kind in kinds:
        e = reg[kind]
        e["proofs_per_s"] = statistics.median(e["region_proofs_per_s"])
        if "latency_ms" in e:
            e["median_submit_to_collect_ms"] = statistics.median(e["latency_ms"])
        print("%-20s %s  median %.1f proofs/s%s" % (kind, " ".join("%.1f" % v for v in e["region_proofs_per_s"]), e["proofs_per_s"],
                                                    "  latency %.2f ms" % e["median_submit_to_collect_ms"] if "latency_ms" in e else ""), flush=True)
    doc["regions"] = reg
    b = reg["b_resident_batch"]["region_proofs_per_s"]
    doc["c_over_b"] = reg["c_queue_resident"]["proofs_per_s"] / reg["b_resident_batch"]["proofs_per_s"]
    doc["e_over_d"] = reg["e_queue_host"]["proofs_per_s"] / reg["d_host_batch"]["proofs_per_s"]
    doc["c_over_a"] = reg["c_queue_resident"]["proofs_per_s"] / reg["a_resident_singles"]["proofs_per_s"]
    doc["b_spread"] = (max(b) - min(b)) / statistics.median(b)
    doc["c_inside_the_spread_of_b"] = min(b) <= reg["c_queue_resident"]["proofs_per_s"] <= max(b)
    print("c / b = %.4f   e / d = %.4f   c / a = %.4f   spread of b's regions %.2f %%" % (doc["c_over_b"], doc["e_over_d"], doc["c_over_a"], 100 * doc["b_spread"]), flush=True)
    pk.close()
    for a in zs:
        a.close()
    cs.close()
    if args.sha_hashes > 0:
        doc["sha256"] = sha_regions(ctx, args, step)
    for name, path in (("bench_parent", args.bench_parent), ("bench_tree", args.bench_tree)):
        if path and os.path.exists(path):
            doc[name] = [json.loads(line) for line in open(path) if line.lstrip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    ctx.close()


def sha_regions(ctx, args, step):
    """(f) the stdlib SHA-256 circuit (a witness of bits: it packs to a fraction of m x 32 B): packed submits through the queue against
    zkhip_assignment_upload_packed + zkhip_prove_g16_resident per proof"""
    from zokrates_amd import sha256_circuit
    steps = args.steps
    with step("sha256 setup"):
        circ = sha256_circuit.circuit(0, args.sha_hashes)
        cs = native.ConstraintSystem(ctx, 0, circ.n, circ.l, circ.w, circ.mats())
        pk = native.ProvingKey(ctx, 0, native.setup_g16(ctx, cs, synth.toxic_waste(0)))
        pk.bind(cs)
        packed = [native.pack_assignment(circ.assignment(0x5EED + i)) for i in range(4)]
    out = {"hashes": args.sha_hashes, "constraints": circ.n, "packed_bytes": int(packed[0].size), "plain_bytes": circ.m * 32,
           "f_upload_packed_then_single": [], "f_queue_packed": [], "latency_ms": []}
    for rep in range(args.repeats + 1):      # (the first round is the warm-up)
        r = [(2000 * rep + j + 1, 9 + j) for j in range(steps)]
        with step("sha region %d singles" % rep):
            t0 = time.perf_counter()
            for j in range(steps):
                a = native.Assignment.from_packed(ctx, cs, packed[j % 4])
                native.prove_g16_resident(ctx, pk, cs, a, *r[j])
                a.close()
            dt_a = time.perf_counter() - t0
        with step("sha region %d queue" % rep):
            with native.ProofQueue(ctx, pk, cs) as q:
                dt_q, lat, _ = queue_region(q, [packed[j % 4] for j in range(steps)], r, packed=True)
        if rep:
            out["f_upload_packed_then_single"].append(steps / dt_a)
            out["f_queue_packed"].append(steps / dt_q)
            out["latency_ms"] += lat
    out["median_submit_to_collect_ms"] = statistics.median(out.pop("latency_ms"))
    print("sha256 x%d: upload_packed + single %.1f proofs/s | queue, packed submits %.1f proofs/s" % (
        args.sha_hashes, statistics.median(out["f_upload_packed_then_single"]), statistics.median(out["f_queue_packed"])), flush=True)
    pk.close()
    cs.close()
    return out


if __name__ == "__main__":
    main()
