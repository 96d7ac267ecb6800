"""A lone witness across the device, measured: the level-scheduled route of `zkhip_compute_witness` (ZKHIP_TUNE_EXEC_WIDE) against the
one-lane route, over the synthetic bit-oriented program of tools/exec_bench.py.

    python tools/exec_wide_bench.py [--log-statements 20] [--instances 1,8,64,1024] [--sweep 64,...,8192] [--out profiles/device_exec_wide.json]

Both routes run in ONE process, alternating, arguments in and resident assignments out (no file, no inputs); every figure is the
median of its repeats with the repeats beside it.  The program's `zkhip_xplan_levels` figures (its DEPTH: the synthetic program is wide
by construction, a deep and narrow one gains only what its depth allows) and the launches per chunk stand beside every time.  Then, at
one instance, a sweep of ZKHIP_TUNE_EXEC_WIDE_MIN, which is what fixes the default."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from exec_bench import build_program  # noqa: E402
from zokrates_amd import native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-statements", type=int, default=20)
    ap.add_argument("--instances", default="1,8,64,1024")
    ap.add_argument("--sweep", default="64,128,256,512,1024,2048,4096,8192")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one-lane-repeats", type=int, default=2, help="the one-lane route takes seconds per call at 2^20 statements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_exec_wide.json"))
    ap.add_argument("--emulator", action="store_true", help="a dry run of this tool on the test-only emulator build (no figure of it means anything)")
    a = ap.parse_args()
    say = lambda *x: print(*x, flush=True)
    t0 = time.time()
    data, counts = build_program(a.log_statements)
    data = np.frombuffer(data, dtype=np.uint8)
    say("program: %d statements, %.1f MB, written in %.1f s" % (sum(counts.values()), data.size / 1e6, time.time() - t0))
    lib = None
    if a.emulator:
        from emu_util import emu_library
        lib = emu_library()
    ctx = native.Context(0, lib)
    prog = native.Program(data, lib)
    cs = prog.constraint_system(ctx)
    t0 = time.time()
    plan = prog.exec_plan(ctx, cs, data)
    t_plan = time.time() - t0
    levels = dict(zip(("levels", "widest_level", "instructions", "levels_below_64"), plan.levels()))
    say("plan in %.2f s: %s" % (t_plan, levels))
    result = {"device": ctx.describe(), "curve": "bn128", "statements": plan.n_statements, "mix": counts, "plan_create_s": round(t_plan, 3), "schedule": levels,
              "how": "zkhip_compute_witness, arguments in, resident assignments out; both routes alternating in one process; seconds, median of the repeats",
              "instances": [], "wide_min_sweep_at_one_instance": []}
    rnd = random.Random(7)
    draw = lambda count: np.frombuffer(b"".join(rnd.randrange(1 << 32).to_bytes(32, "little") for _ in range(count * 4)), dtype=np.uint8)

    def timed(args, wide, wide_min=0):
        ctx.tune("exec_wide", wide)
        ctx.tune("exec_wide_min", wide_min)
        t0 = time.time()
        got = ctx.compute_witness(plan, args)
        dt = time.time() - t0
        assert got.code == 0
        got.close()
        last = ctx.exec_last()
        assert last[0] == 1 + wide
        return dt, last

    def dump():
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    # one small call of each route first: the code objects are loaded and the stream made outside the timed calls
    timed(draw(1), 0)
    timed(draw(1), 1)
    for count in [int(x) for x in a.instances.split(",")]:
        args = draw(count)
        one, wide, last = [], [], None
        for k in range(max(a.repeats, a.one_lane_repeats)):
            if k < a.one_lane_repeats:
                one.append(timed(args, 0)[0])
            if k < a.repeats:
                dt, last = timed(args, 1)
                wide.append(dt)
        rec = {"instances": count, "one_lane_s": round(statistics.median(one), 5), "wide_s": round(statistics.median(wide), 5),
               "one_lane_over_wide": round(statistics.median(one) / statistics.median(wide), 2), "one_lane_repeats_s": [round(x, 5) for x in one],
               "wide_repeats_s": [round(x, 5) for x in wide], "chunks": last[1], "launches_per_chunk": last[2], "wide_min": last[3], "levels": levels["levels"]}
        say(json.dumps(rec))
        result["instances"].append(rec)
        dump()
    args = draw(1)
    for wide_min in [int(x) for x in a.sweep.split(",")]:
        times, last = [], None
        for _ in range(a.repeats):
            dt, last = timed(args, 1, wide_min)
            times.append(dt)
        rec = {"wide_min": wide_min, "wide_s": round(statistics.median(times), 5), "repeats_s": [round(x, 5) for x in times], "launches_per_chunk": last[2],
               "levels": levels["levels"]}
        say(json.dumps(rec))
        result["wide_min_sweep_at_one_instance"].append(rec)
        dump()
    ctx.tune("exec_wide", 0)
    ctx.tune("exec_wide_min", 0)
    plan.close()
    cs.close()
    prog.close()
    ctx.close()


if __name__ == "__main__":
    main()
