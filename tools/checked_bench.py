#!/usr/bin/env python3
"""Checked proving against unchecked proving on one device, in ONE process: the dense synthetic circuit on bn128, Groth16,
resident assignments — over the key as loaded (unbound: six transforms) and bound to its constraint system (four), the state
`bench.py` times.

    python tools/checked_bench.py [--log-domain 20] [--steps 20] [--repeats 3] [--singles 7] [--step-limit 240] [--out profiles/checked_mode.json]

The timed regions ALTERNATE (unchecked, checked, unchecked, checked, ...) so that whatever else the box is doing falls on both.
A region is one `zkhip_prove_g16_resident_batch` call over `--steps` proofs, after a lone proof and a batch of four as warm-up
(every proof slot allocates its workspaces at first use); the single-proof figures are wall clocks of lone resident proofs,
alternating the same way; `zkhip_r1cs_check` alone is timed from a resident assignment.  Every step runs under `--step-limit`
seconds: a step that overruns ends the process with status 3 and nothing after it is started.  Writes one JSON document."""
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
        sys.stderr.write("checked_bench: step '%s' exceeded %d s: stopping\n" % (self.what, self.seconds))
        sys.stderr.flush()
        os._exit(3)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._late)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-domain", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--singles", type=int, default=7)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checked_mode.json"))
    args = ap.parse_args()
    step = lambda what: StepLimit(args.step_limit, what)
    cid, lg, nw = 0, args.log_domain, 4
    ctx = native.Context(args.device)
    doc = {"tool": "tools/checked_bench.py", "device": ctx.describe(), "workload": "synthetic R1CS dense, bn128, Groth16, resident assignments",
           "log_domain": lg, "steps_per_region": args.steps, "regions_per_mode": args.repeats, "order": "regions alternate unchecked, checked", "keys": {}}
    with step("setup"):
        circ = synth.circuit(cid, lg, kind="dense", seed=0xABCD + lg)
        cs = native.ConstraintSystem(ctx, cid, circ.n, circ.l, circ.w, circ.mats())
        raw = native.setup_g16(ctx, cs, synth.toxic_waste(cid))
    with step("key load"):
        pk = native.ProvingKey(ctx, cid, raw)
        del raw
        zs = [native.Assignment(ctx, cs, circ.assignment(0x5EED + lg + i)) for i in range(nw)]
    doc["constraints"] = circ.n
    with step("zkhip_r1cs_check alone"):
        assert cs.check(zs[0]) == (None, 0)
        alone = []
        for k in range(max(args.singles, 5)):
            t0 = time.perf_counter()
            cs.check(zs[k % nw])
            alone.append(1e3 * (time.perf_counter() - t0))
    doc["r1cs_check_resident_ms"] = {"samples": alone, "median": statistics.median(alone)}
    print("zkhip_r1cs_check alone, resident assignment, 2^%d: %.3f ms" % (lg, statistics.median(alone)), flush=True)
    for key_state in ("unbound", "bound"):
        if key_state == "bound":
            with step("bind"):
                pk.bind(cs)
                assert pk.is_bound(cs)
        entry = {m: {"region_proofs_per_s": [], "single_ms": []} for m in ("unchecked", "checked")}
        with step("warm-up " + key_state):
            want = native.prove_g16_resident(ctx, pk, cs, zs[0], 11, 13)
            for on in (False, True):
                ctx.set_checked(on)
                assert native.prove_g16_resident(ctx, pk, cs, zs[0], 11, 13) == want, "checked and unchecked proofs differ"
                native.prove_g16_resident_batch(ctx, pk, cs, [zs[i % nw] for i in range(4)], [(100 + i, 200 + i) for i in range(4)])
        for rep in range(args.repeats):
            for mode in ("unchecked", "checked"):
                ctx.set_checked(mode == "checked")
                with step("region %d %s %s" % (rep, key_state, mode)):
                    aa = [zs[j % nw] for j in range(args.steps)]
                    rs = [(1000 * rep + j, 7 + j) for j in range(args.steps)]
                    t0 = time.perf_counter()
                    native.prove_g16_resident_batch(ctx, pk, cs, aa, rs)
                    dt = time.perf_counter() - t0
                entry[mode]["region_proofs_per_s"].append(args.steps / dt)
        for k in range(args.singles):
            for mode in ("unchecked", "checked"):
                ctx.set_checked(mode == "checked")
                with step("single %d %s %s" % (k, key_state, mode)):
                    t0 = time.perf_counter()
                    native.prove_g16_resident(ctx, pk, cs, zs[k % nw], 31 + k, 37 + k)
                    entry[mode]["single_ms"].append(1e3 * (time.perf_counter() - t0))
        ctx.set_checked(False)
        for mode in ("unchecked", "checked"):
            entry[mode]["proofs_per_s"] = statistics.median(entry[mode]["region_proofs_per_s"])
            entry[mode]["single_proof_ms"] = statistics.median(entry[mode]["single_ms"])
        entry["ratio_proofs_per_s_checked_over_unchecked"] = entry["checked"]["proofs_per_s"] / entry["unchecked"]["proofs_per_s"]
        entry["single_proof_ms_checked_minus_unchecked"] = entry["checked"]["single_proof_ms"] - entry["unchecked"]["single_proof_ms"]
        doc["keys"][key_state] = entry
        print("%s: unchecked %.1f proofs/s, %.3f ms single | checked %.1f proofs/s, %.3f ms single | ratio %.4f" % (
            key_state, entry["unchecked"]["proofs_per_s"], entry["unchecked"]["single_proof_ms"], entry["checked"]["proofs_per_s"],
            entry["checked"]["single_proof_ms"], entry["ratio_proofs_per_s_checked_over_unchecked"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
