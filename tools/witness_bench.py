#!/usr/bin/env python3
"""Witness files read on the device against the host reader, on one device, in ONE process: what handing the bytes of a ZoKrates
`witness` file to the device (`zkhip_assignment_upload_witness`, `zkhip_queue_submit_witness`: 40 B per entry copied, two launches)
costs or gains against `zkhip_prog_assignment` on the calling thread followed by the plain upload (32 B per variable copied).
Two workloads, both bn128 / Groth16, the key bound to its system, the stream plan, 16 hardware queues asked for: stdlib SHA-256 as
`bench.py` shapes it (21 compressions side by side, m ~ 1.02 M, a witness of bits) and the dense synthetic circuit at 2^20.

    python tools/witness_bench.py [--log-domain 20] [--steps 20] [--regions 3] [--step-limit 240] [--out profiles/witness_ingest.json]

Per workload:
  (a) host_reader_ms         zkhip_prog_assignment alone (witness file -> z and inputs in host memory)
  (b) to_resident_ms         zkhip_prog_assignment + zkhip_assignment_upload against zkhip_assignment_upload_witness, each to its verdict
                             (the allocation of the (m + 2) x 32 B device buffer is inside the clock on both sides, freeing it outside)
  (c) queue_proofs_per_s     the queue's steady state from witness BYTES: zkhip_prog_assignment + zkhip_queue_submit per proof against
                             zkhip_queue_submit_witness, collects through zkhip_queue_collect_inputs on the device side
  (d) lone_proof_ms          one proof from witness bytes: zkhip_prog_assignment + zkhip_prove_g16 against
                             zkhip_assignment_upload_witness + zkhip_prove_g16_resident
The two sides of (b), (c) and (d) ALTERNATE region by region — `--regions` regions of `--steps` calls each per side — so whatever else
the box is doing falls on both; a figure is the median over a side's calls (b, d: wall clocks of single calls; c: proofs/s of whole
regions).  Every ratio's baseline is the host-reader side of the same process.  The calls go through ctypes with every output buffer
allocated and touched beforehand: no allocation or zero-fill of the binding is inside a clock.  Every step runs under `--step-limit`
seconds: one that overruns ends the process with status 3 and nothing after it is started.  A run on the test emulator
(ZKHIP_LIBRARY) only rehearses the tool: its timings mean nothing and no file is written."""
import argparse
import ctypes as C
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
        sys.stderr.write("witness_bench: step '%s' exceeded %d s: stopping\n" % (self.what, self.seconds))
        sys.stderr.flush()
        os._exit(3)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._late)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def summary(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": [round(x, 4) for x in samples]}


class Routes:
    """The two routes from the bytes of a witness file, over raw ctypes calls and buffers made once."""

    def __init__(self, ctx, prog, cs, pk, plan, wits):
        self.L, self.ctx, self.prog, self.cs, self.pk, self.plan = ctx.lib.L, ctx, prog, cs, pk, plan
        self.wits = [np.ascontiguousarray(w, dtype=np.uint8) for w in wits]
        self.z = np.ones(prog.m * 32, dtype=np.uint8)                      # (ones: every page touched)
        self.cap = prog.n_public_args + prog.return_count + 8
        self.inputs = np.ones(self.cap * 32, dtype=np.uint8)
        self.proof = np.ones(8 * 32 + 3, dtype=np.uint8)
        self.n_in = C.c_uint64()

    def ok(self, rc):
        if rc != 0:
            raise native.ZkhipError(rc, self.L.zkhip_last_error(self.ctx.h).decode() or self.L.zkhip_last_error(None).decode())

    def rnd(self, k):
        return np.frombuffer((1000 + k).to_bytes(32, "little") + (7 + k).to_bytes(32, "little"), dtype=np.uint8)

    def read(self, k):
        w = self.wits[k % len(self.wits)]
        self.ok(self.L.zkhip_prog_assignment(self.prog.h, native._ptr(w), w.size, native._ptr(self.z), native._ptr(self.inputs), self.cap, C.byref(self.n_in)))

    def host_resident(self, k):
        self.read(k)
        a = C.c_void_p()
        self.ok(self.L.zkhip_assignment_upload(self.ctx.h, self.cs.h, native._ptr(self.z), C.byref(a)))
        return a

    def device_resident(self, k):
        w = self.wits[k % len(self.wits)]
        a = C.c_void_p()
        self.ok(self.L.zkhip_assignment_upload_witness(self.ctx.h, self.plan.h, native._ptr(w), w.size, native._ptr(self.inputs), self.cap, C.byref(self.n_in), C.byref(a)))
        return a

    def free(self, a):
        if a:
            self.L.zkhip_assignment_free(a)

    def host_lone(self, k):
        self.read(k)
        r = self.rnd(k)
        self.ok(self.L.zkhip_prove_g16(self.ctx.h, self.pk.h, self.cs.h, native._ptr(self.z), native._ptr(r), native._ptr(r[32:]), native._ptr(self.proof), None))

    def device_lone(self, k):
        a = self.device_resident(k)
        r = self.rnd(k)
        self.ok(self.L.zkhip_prove_g16_resident(self.ctx.h, self.pk.h, self.cs.h, a, native._ptr(r), native._ptr(r[32:]), native._ptr(self.proof), None))
        return a

    def queue_region(self, device, steps, base):
        """`steps` proofs through a fresh queue in the steady state, from witness bytes; (seconds, proofs)"""
        proofs = []
        ticket = C.c_uint64()
        with native.ProofQueue(self.ctx, self.pk, self.cs) as q:
            cap, flying = q.state()[0], 0

            def collect():
                if device:
                    self.ok(self.L.zkhip_queue_collect_inputs(q.h, C.byref(ticket), native._ptr(self.proof), native._ptr(self.inputs), self.cap, C.byref(self.n_in), None))
                else:
                    self.ok(self.L.zkhip_queue_collect(q.h, C.byref(ticket), native._ptr(self.proof), None))
                proofs.append(self.proof.tobytes())

            t0 = time.perf_counter()
            for k in range(steps):
                if flying == cap:
                    collect()
                    flying -= 1
                r = self.rnd(base + k)
                if device:
                    w = self.wits[(base + k) % len(self.wits)]
                    self.ok(self.L.zkhip_queue_submit_witness(q.h, self.plan.h, native._ptr(w), w.size, native._ptr(r), C.byref(ticket)))
                else:
                    self.read(base + k)
                    self.ok(self.L.zkhip_queue_submit(q.h, native._ptr(self.z), None, native._ptr(r), C.byref(ticket)))
                flying += 1
            while flying:
                collect()
                flying -= 1
            dt = time.perf_counter() - t0
        return dt, proofs


def timed(fn, k, after=None):
    t0 = time.perf_counter()
    out = fn(k)
    dt = 1e3 * (time.perf_counter() - t0)
    if after:
        after(out)
    return dt


def workload(ctx, name, circ, zs, args, step):
    cid, steps, regions = 0, args.steps, args.regions
    m = circ.m
    rec = {"constraints": circ.n, "variables": m}
    with step(name + ": program, system, setup, key, bind, plan"):
        ids = np.arange(m, dtype=np.int64)
        prog = native.Program(native.write_program(cid, circ.n, m, circ.mats(), ids=ids, args=[(j, False) for j in range(1, circ.l)]))
        assert (prog.m, prog.l) == (m, circ.l)
        cs = prog.constraint_system(ctx)
        pk = native.ProvingKey(ctx, cid, native.setup_g16(ctx, cs, synth.toxic_waste(cid)))
        pk.bind(cs)
        assert pk.is_bound(cs)
        plan = prog.plan(ctx, cs)
        wits = [native.write_witness(ids, z) for z in zs]
    rec["bytes"] = {"witness_file": int(wits[0].size), "assignment": 32 * m, "file_over_assignment": wits[0].size / (32 * m)}
    rt = Routes(ctx, prog, cs, pk, plan, wits)
    with step(name + ": same bytes"):
        for k in range(len(wits)):
            rt.read(k)
            assert rt.z.tobytes() == zs[k].tobytes()
            want_inputs = rt.inputs[:32 * rt.n_in.value].tobytes()
            rt.host_lone(k)
            want = rt.proof.tobytes()
            a = rt.device_lone(k)
            assert rt.proof.tobytes() == want and rt.inputs[:32 * rt.n_in.value].tobytes() == want_inputs, "the device route's proof or inputs differ"
            rt.free(a)
        assert rt.queue_region(True, 4, 0)[1] == rt.queue_region(False, 4, 0)[1], "the queue's proofs differ between the routes"
    with step(name + ": (a) host reader"):
        for k in range(2):
            rt.read(k)
        rec["host_reader_ms"] = summary([timed(rt.read, k) for k in range(regions * steps)])
    sides = (("host_reader", False), ("device", True))
    with step(name + ": (b) to a resident assignment"):
        s = {"host_reader": [], "device": []}
        for rep in range(regions + 1):      # (the first round is the warm-up)
            for side, device in sides:
                got = [timed(rt.device_resident if device else rt.host_resident, rep * steps + k, rt.free) for k in range(steps)]
                if rep:
                    s[side] += got
        rec["to_resident_ms"] = {k: summary(v) for k, v in s.items()}
    with step(name + ": (c) queue"):
        s = {"host_reader": [], "device": []}
        for rep in range(regions + 1):
            for side, device in sides:
                dt, _ = rt.queue_region(device, steps, rep * steps)
                if rep:
                    s[side].append(steps / dt)
        rec["queue_proofs_per_s"] = {k: summary(v) for k, v in s.items()}
    with step(name + ": (d) lone proofs"):
        s = {"host_reader": [], "device": []}
        for rep in range(regions + 1):
            for side, device in sides:
                got = [timed(rt.device_lone if device else rt.host_lone, rep * steps + k, rt.free if device else None) for k in range(steps)]
                if rep:
                    s[side] += got
        rec["lone_proof_ms"] = {k: summary(v) for k, v in s.items()}
    med = lambda key, side: rec[key][side]["median"]
    rec["ratios_device_over_host_reader"] = {key: med(key, "device") / med(key, "host_reader") for key in ("to_resident_ms", "queue_proofs_per_s", "lone_proof_ms")}
    print("%s: m %d | host reader %.3f ms | to resident %.3f -> %.3f ms | queue %.1f -> %.1f proofs/s | lone proof %.3f -> %.3f ms" % (
        name, m, rec["host_reader_ms"]["median"], med("to_resident_ms", "host_reader"), med("to_resident_ms", "device"),
        med("queue_proofs_per_s", "host_reader"), med("queue_proofs_per_s", "device"), med("lone_proof_ms", "host_reader"), med("lone_proof_ms", "device")), flush=True)
    plan.close()
    pk.close()
    cs.close()
    prog.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-domain", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bench-parent", default=None, help="file with bench.py's result lines on the parent commit")
    ap.add_argument("--bench-tree", default=None, help="file with bench.py's result lines on this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_ingest.json"))
    args = ap.parse_args()
    step = lambda what: StepLimit(args.step_limit, what)
    lg = args.log_domain
    native.default_library().init(16)
    ctx = native.Context(args.device)
    ctx.tune("pipe_plan", 1)
    desc = ctx.describe()
    rehearsal = "EMULATOR" in desc
    if not rehearsal and (args.steps < 20 or args.regions < 3):
        sys.exit("at least three regions of 20 per side")
    doc = {"tool": "tools/witness_bench.py", "device": desc, "host": os.uname().nodename, "log_domain": lg, "steps_per_region": args.steps,
           "regions_per_side": args.regions, "hw_queues_requested": 16, "pipe_plan": 1,
           "order": "the two sides of (b), (c), (d) alternate region by region after one warm-up region each, one process; medians",
           "scheme": "Groth16, bn128, key bound to its constraint system", "workloads": {}}
    with step("circuits"):
        per_hash = len(sha.template()[0])
        c_sha = sha.circuit(0, max(1, (1 << lg) // (per_hash + 7)))
        z_sha = [c_sha.assignment(0x5EED + i) for i in range(3)]
        c_dense = synth.circuit(0, lg, kind="dense", seed=0xABCD + lg)
        z_dense = [c_dense.assignment(0x5EED + lg + i) for i in range(3)]
    print("circuits: sha256_stdlib %d hashes, m %d; dense m %d" % (c_sha.hashes, c_sha.m, c_dense.m), flush=True)
    doc["workloads"]["sha256_stdlib"] = dict(workload(ctx, "sha256_stdlib", c_sha, z_sha, args, step), hashes=c_sha.hashes)
    doc["workloads"]["dense"] = workload(ctx, "dense", c_dense, z_dense, args, step)
    ctx.close()
    if rehearsal:
        print("rehearsal on the emulator: the timings mean nothing, nothing is written")
        return
    for name, path in (("bench_parent", args.bench_parent), ("bench_tree", args.bench_tree)):
        if path and os.path.exists(path):
            doc[name] = [json.loads(line) for line in open(path) if line.lstrip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
