#!/usr/bin/env python3
"""BLS12-377 against BLS12-381 on one device, in ONE process: the same dense synthetic circuit at 2^18 and 2^20 constraints,
Groth16 over a key bound to its constraint system, resident assignments — the state `bench.py` times.

    python tools/curve_bench.py [--log-domains 18,20] [--steps 20] [--repeats 3] [--step-limit 240] [--out profiles/bls377_vs_bls381.json]

Per size both curves' keys are resident together and the timed regions ALTERNATE between them (381, 377, 381, 377, ...), so that
whatever else the box is doing falls on both.  A region is one `zkhip_prove_g16_resident_batch` call over `--steps` proofs (after a
lone proof and a batch of four as warm-up: every proof slot allocates its workspaces at first use); the single-proof figures are the
library's own event timings of lone resident proofs (total, and the bucket accumulation kernel of the G2 lane, k_msm_accum<G2>).
Every step (setup, key load, bind, warm-up, each region) runs under `--step-limit` seconds: a step that overruns ends the process
with status 3 and nothing after it is started.  Writes one JSON document; the ratio to hold is proofs/s(377) >= 0.90 x proofs/s(381)."""
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

CURVES = ((1, "bls12_381"), (2, "bls12_377"))


class StepLimit:
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _late(self, *_):
        sys.stderr.write("curve_bench: step '%s' exceeded %d s: stopping\n" % (self.what, self.seconds))
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
    ap.add_argument("--log-domains", default="18,20")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--singles", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls377_vs_bls381.json"))
    args = ap.parse_args()
    step = lambda what: StepLimit(args.step_limit, what)
    ctx = native.Context(args.device)
    doc = {"tool": "tools/curve_bench.py", "device": ctx.describe(), "workload": "synthetic R1CS dense, Groth16, key bound to the constraint system, resident assignments",
           "steps_per_region": args.steps, "regions_per_curve": args.repeats, "order": "regions alternate bls12_381, bls12_377", "sizes": []}
    nw = 4
    for lg in (int(x) for x in args.log_domains.split(",")):
        entry = {"log_domain": lg, "curves": {}}
        state = {}
        for cid, name in CURVES:
            with step("setup %s 2^%d" % (name, lg)):
                circ = synth.circuit(cid, lg, kind="dense", seed=0xABCD + lg)
                cs = native.ConstraintSystem(ctx, cid, circ.n, circ.l, circ.w, circ.mats())
                raw = native.setup_g16(ctx, cs, synth.toxic_waste(cid))
            with step("key load and bind %s 2^%d" % (name, lg)):
                pk = native.ProvingKey(ctx, cid, raw)
                del raw
                zs = [native.Assignment(ctx, cs, circ.assignment(0x5EED + lg + i)) for i in range(nw)]
                unbound = native.prove_g16_resident(ctx, pk, cs, zs[0], 11, 13)
                pk.bind(cs)
                assert pk.is_bound(cs) and native.prove_g16_resident(ctx, pk, cs, zs[0], 11, 13) == unbound, "bound and unbound proofs differ"
            with step("warm-up %s 2^%d" % (name, lg)):
                native.prove_g16_resident_batch(ctx, pk, cs, [zs[i % nw] for i in range(4)], [(100 + i, 200 + i) for i in range(4)])
            state[cid] = (circ, cs, pk, zs)
            entry["curves"][name] = {"constraints": circ.n, "region_proofs_per_s": [], "single_total_ms": [], "single_accum_g2_ms": [], "single_accum_g1_ms": []}
        for rep in range(args.repeats):
            for cid, name in CURVES:
                circ, cs, pk, zs = state[cid]
                with step("region %d %s 2^%d" % (rep, name, lg)):
                    aa = [zs[j % nw] for j in range(args.steps)]
                    rs = [(1000 * rep + j, 7 + j) for j in range(args.steps)]
                    t0 = time.perf_counter()
                    native.prove_g16_resident_batch(ctx, pk, cs, aa, rs)
                    dt = time.perf_counter() - t0
                entry["curves"][name]["region_proofs_per_s"].append(args.steps / dt)
        for k in range(args.singles):
            for cid, name in CURVES:
                circ, cs, pk, zs = state[cid]
                with step("single %d %s 2^%d" % (k, name, lg)):
                    _, tm = native.prove_g16_resident(ctx, pk, cs, zs[k % nw], 31 + k, 37 + k, want_timings=True)
                c = entry["curves"][name]
                c["single_total_ms"].append(tm["total_ms"])
                c["single_accum_g2_ms"].append(tm["kernel_msm_accum_g2_ms"])
                c["single_accum_g1_ms"].append(tm["kernel_msm_accum_g1_ms"])
        for cid, name in CURVES:
            c = entry["curves"][name]
            c["proofs_per_s"] = statistics.median(c["region_proofs_per_s"])
            c["single_proof_ms"] = statistics.median(c["single_total_ms"])
            c["k_msm_accum_g2_ms"] = statistics.median(c["single_accum_g2_ms"])
            c["k_msm_accum_g1_ms"] = statistics.median(c["single_accum_g1_ms"])
        a, b = entry["curves"]["bls12_377"], entry["curves"]["bls12_381"]
        entry["ratio_proofs_per_s_377_over_381"] = a["proofs_per_s"] / b["proofs_per_s"]
        entry["ratio_k_msm_accum_g2_381_over_377"] = b["k_msm_accum_g2_ms"] / a["k_msm_accum_g2_ms"]
        entry["expectation_0_90_met"] = entry["ratio_proofs_per_s_377_over_381"] >= 0.90
        doc["sizes"].append(entry)
        print("2^%d: bls12_381 %.1f proofs/s, %.2f ms single, accum G2 %.2f ms | bls12_377 %.1f proofs/s, %.2f ms single, accum G2 %.2f ms | ratio %.3f" % (
            lg, b["proofs_per_s"], b["single_proof_ms"], b["k_msm_accum_g2_ms"], a["proofs_per_s"], a["single_proof_ms"], a["k_msm_accum_g2_ms"],
            entry["ratio_proofs_per_s_377_over_381"]), flush=True)
        for cid, _ in CURVES:
            circ, cs, pk, zs = state[cid]
            for z in zs:
                z.close()
            pk.close()
            cs.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
