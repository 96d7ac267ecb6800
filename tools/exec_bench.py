"""Witnesses computed on the device, measured: `zkhip_compute_witness` over a synthetic bit-oriented program.

    python tools/exec_bench.py [--log-statements 20] [--batches 64,1024,4096] [--out profiles/device_exec.json]

The program (about 2^LOG statements over BN254, four 32-bit arguments, one output) has the statement mix of a circuit that works on
bits — what a hash compiles to:

    2 %  Bits(32) of a sum of earlier words         30 %  Xor of two earlier bits          10 %  ShaCh of three bits
   10 %  ShaAndXorAndXorAnd (majority) of three      2 %  Or                                1 %  ConditionEq / Div / EuclideanDiv
   20 %  checks  b * b == b  on an earlier bit      25 %  defines: a word from up to 32 bits with powers of two as coefficients, times one

Every statement holds for every argument list, so each instance runs through.  Per batch it records the time of
`zkhip_compute_witness` to RESIDENT ASSIGNMENTS (no file, no inputs), statements per second (statements executed x instances / time),
the bytes of the value store, and beside it the route the call replaces in this project: `zkhip_assignment_upload_witness` of the same
witnesses from host bytes, timed over a SAMPLE of the batch's witness files (a batch of files does not fit host memory: 40 B per entry
per instance) and scaled to the batch.  The reference's interpreter (Rust) cannot be built where this runs: no figure is quoted for it.

The writer below assembles the `out` bytes from fragments (a million statements through a generic encoder take minutes); its first
statements are held against `tests/serde_model.py`'s encoder byte for byte before anything is timed."""
import argparse
import json
import os
import random
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from oracle.fields import BN254  # noqa: E402
from zokrates_amd import native  # noqa: E402

R = BN254.r


# ---------------- the fragment writer ----------------
def head(major, n):
    if n < 24:
        return bytes([major << 5 | n])
    for ai, fmt, lim in ((24, ">B", 1 << 8), (25, ">H", 1 << 16), (26, ">I", 1 << 32), (27, ">Q", 1 << 64)):
        if n < lim:
            return bytes([major << 5 | ai]) + struct.pack(fmt, n)
    raise ValueError(n)


def text(s):
    return head(3, len(s)) + s.encode()


SPAN = text("span") + b"\xf6"
VAR = head(5, 1) + text("id")
_coeff = {}


def var(v):
    return VAR + (head(0, v) if v >= 0 else head(1, -1 - v))


def coeff(c):
    b = _coeff.get(c)
    if b is None:
        b = _coeff[c] = head(2, 32) + int(c % R).to_bytes(32, "little")
    return b


def lc(terms):
    return head(5, 2) + SPAN + text("value") + head(4, len(terms)) + b"".join(head(4, 2) + var(v) + coeff(c) for v, c in terms)


ONE = lc([(0, 1)])


def quad(left, right=None):
    return head(5, 3) + SPAN + text("left") + lc(left) + text("right") + (ONE if right is None else lc(right))


CONSTRAINT = head(5, 1) + text("Constraint") + head(5, 4) + SPAN + text("quad")
DIRECTIVE = head(5, 1) + text("Directive") + head(5, 4) + SPAN + text("inputs")


def constraint(left, right, lin):
    return CONSTRAINT + quad(left, right) + text("lin") + lc(lin) + text("error") + b"\xf6"


def directive(inputs, outputs, solver):
    sv = text(solver) if isinstance(solver, str) else head(5, 1) + text(solver[0]) + head(0, solver[1])
    return DIRECTIVE + head(4, len(inputs)) + b"".join(quad(l, r) for l, r in inputs) + text("outputs") + head(4, len(outputs)) + b"".join(var(o) for o in outputs) + text("solver") + sv


def model_statement(kind, *a):
    """the same statement as tests/exec_ref.py describes it, for the byte-for-byte comparison"""
    import exec_ref as X
    if kind == "c":
        return X.constraint(a[0], a[1] if a[1] is not None else [(0, 1)], a[2])
    return X.directive([(l, r if r is not None else [(0, 1)]) for l, r in a[0]], a[1], a[2])


def build_program(log_statements, seed=0xB17):
    """(`out` bytes, description of the mix as counted)"""
    rnd = random.Random(seed)
    target = 1 << log_statements
    n_args = 4
    words = list(range(1, n_args + 1))      # variables that hold 32-bit words
    bits = []
    nxt = [n_args + 1]
    blobs, described, counts = [], [], {}

    def fresh(k=1):
        v = list(range(nxt[0], nxt[0] + k))
        nxt[0] += k
        return v

    def emit(name, kind, *a):
        counts[name] = counts.get(name, 0) + 1
        blobs.append(constraint(*a) if kind == "c" else directive(*a))
        if len(described) < 300:
            described.append((kind, a))

    # the arguments' bits first: everything else draws on them
    for w in list(words):
        outs = fresh(32)
        emit("Bits(32)", "d", [([(w, 1)], None)], outs, ("Bits", 32))
        bits.extend(outs)
    while len(blobs) < target - 1:
        x = rnd.random()
        pick = lambda: rnd.choice(bits[-4096:]) if rnd.random() < 0.8 else rnd.choice(bits)
        if x < 0.02:
            outs = fresh(32)
            emit("Bits(32)", "d", [([(rnd.choice(words[-64:]), 1)], None)], outs, ("Bits", 32))
            bits.extend(outs)
        elif x < 0.32:
            o = fresh()
            emit("Xor", "d", [([(pick(), 1)], None), ([(pick(), 1)], None)], o, "Xor")
            bits.extend(o)
        elif x < 0.42:
            o = fresh()
            emit("ShaCh", "d", [([(pick(), 1)], None) for _ in range(3)], o, "ShaCh")
            bits.extend(o)
        elif x < 0.52:
            o = fresh()
            emit("ShaAndXorAndXorAnd", "d", [([(pick(), 1)], None) for _ in range(3)], o, "ShaAndXorAndXorAnd")
            bits.extend(o)
        elif x < 0.54:
            o = fresh()
            emit("Or", "d", [([(pick(), 1)], None), ([(pick(), 1)], None)], o, "Or")
            bits.extend(o)
        elif x < 0.55:
            which = rnd.choice(["ConditionEq", "Div", "EuclideanDiv"])
            a, b = rnd.choice(words[-64:]), rnd.choice(words[-64:])
            if which == "ConditionEq":
                emit(which, "d", [([(a, 1), (b, R - 1)], None)], fresh(2), which)
            else:
                emit(which, "d", [([(a, 1)], None), ([(b, 1)], None)], fresh(1 if which == "Div" else 2), which)
        elif x < 0.75:
            b = pick()
            emit("check b*b == b", "c", [(b, 1)], [(b, 1)], [(b, 1)])
        else:
            k = rnd.choice([2, 8, 32, 32])
            w = fresh()
            emit("define a word", "c", [(pick(), 1 << i) for i in range(k)], None, [(w[0], 1)])
            words.extend(w)
    emit("define the output", "c", [(words[-1], 1)], [(words[-2], 1)], [(-1, 1)])
    # the fragments against the table-driven encoder, statement by statement
    import serde_model
    for blob, (kind, a) in zip(blobs, described):
        assert blob == serde_model.encode(serde_model.Statement, model_statement(kind, *a)), "the fragment writer disagrees with tests/serde_model.py"
    params = head(4, n_args) + b"".join(head(5, 3) + SPAN + text("id") + var(v) + text("private") + (b"\xf5" if v > 1 else b"\xf4") for v in range(1, n_args + 1))
    stmts = b"".join(blobs)
    solv, modmap = head(4, 0), head(5, 1) + text("modules") + head(5, 0)
    off, secs = 120, b""
    for ty, blob in ((1, params), (2, stmts), (3, solv), (3, modmap)):
        secs += struct.pack("<IQQ", ty, off, len(blob))
        off += len(blob)
    n_constraints = sum(v for k, v in counts.items() if k in ("check b*b == b", "define a word", "define the output"))
    header = b"ZOK\0" + bytes([3, 0, 0, 0]) + serde_model.field_id(R) + struct.pack("<II", n_constraints, 1) + secs
    return header + b"\0" * (120 - len(header)) + params + stmts + solv + modmap, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-statements", type=int, default=20)
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--sample", type=int, default=4, help="witness files per batch that the upload route is timed over")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_exec.json"))
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
    t0 = time.time()
    prog = native.Program(data, lib)
    cs = prog.constraint_system(ctx)
    t_parse = time.time() - t0
    t0 = time.time()
    plan = prog.exec_plan(ctx, cs, data)
    t_plan = time.time() - t0
    wplan = prog.plan(ctx, cs)
    say("parsed in %.2f s, plan in %.2f s: dims %s" % (t_parse, t_plan, plan.dims))
    result = {"device": ctx.describe(), "curve": "bn128", "statements": plan.n_statements, "mix": counts, "constraints": prog.n, "variables": prog.m,
              "plan": dict(zip(native.ExecPlan.DIMS, plan.dims)), "plan_create_s": round(t_plan, 3), "program_parse_and_upload_s": round(t_parse, 3),
              "reference_interpreter": "not run: the reference (Rust) cannot be built on this machine", "batches": []}
    rnd = random.Random(7)
    # one small call first: the kernels' code objects are loaded and the streams made outside the timed calls
    ctx.compute_witness(plan, [[rnd.randrange(1 << 32) for _ in range(4)]]).close()
    for count in [int(x) for x in a.batches.split(",")]:
        args = np.frombuffer(b"".join(rnd.randrange(1 << 32).to_bytes(32, "little") for _ in range(count * 4)), dtype=np.uint8)
        need = count * (prog.m + 2) * 32
        rec = {"instances": count, "assignment_bytes": need}
        try:
            t0 = time.time()
            got = ctx.compute_witness(plan, args)
            dt = time.time() - t0
            assert got.code == 0
            rec.update({"compute_witness_s": round(dt, 4), "statements_per_s": round(plan.n_statements * count / dt),
                        "instances_per_s": round(count / dt, 2), "value_store_bytes_per_instance": plan.store_bytes})
            got.close()
            del got
            # the route it replaces here: the same witnesses as `witness` files from host bytes, over a sample
            k = min(a.sample, count)
            files = ctx.compute_witness(plan, args[:k * 4 * 32], want_files=True, want_assignments=False).files
            t0 = time.time()
            for f in files:
                ctx.upload_witness(wplan, np.frombuffer(f, dtype=np.uint8), want_inputs=False).close()
            du = (time.time() - t0) / k
            rec.update({"upload_witness_s_per_file": round(du, 5), "upload_witness_s_scaled_to_batch": round(du * count, 3), "witness_file_bytes": len(files[0]),
                        "upload_sample": k})
        except native.ZkhipError as e:
            rec["error"] = str(e)
        say(json.dumps(rec))
        result["batches"].append(rec)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    plan.close()
    wplan.close()
    cs.close()
    prog.close()
    ctx.close()


if __name__ == "__main__":
    main()
