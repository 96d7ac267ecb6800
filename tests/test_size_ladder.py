"""Every domain size from 2^0 to 2^22 held to the oracle: transforms, witness map and proofs, the ad-hoc MSM at every width.

The rungs, the shape model and the check functions are in tests/size_ladder.py.  Each of (b) transforms, (c) proofs and (d) ad-hoc
MSMs has an emulator half (CPU suite: the rungs up to EMU_*, where the emulator stops being cheap) and a `gpu` half that runs every
rung through the same check function.  (a) `test_the_ladder_covers_every_shape` needs no library: it asserts, on the model, that
the rungs taken together reach every window width, every sub-transform length and every pass structure — if a default changes and
a rung moves off its boundary, that test fails and the rung lists are edited.

Comparisons are byte-exact against oracle.cpu, tests/bls377_ref.py or a closed form; the parametrise ids name the curve and the
size.  The ladder runs on the library's defaults; the cases named `tuned` or `forced` reach what no default reaches (short
sub-transforms, three passes below 2^23, the widths the ad-hoc rule never picks, 2-bit windows over a key's tables) through
zkhip_ctx_tune on a context of their own.

BLS12-377 (curve 2) has only the Python reference, whose closed form evaluates the QAP (the SAP, twice as long, for GM17) at the
trapdoor in big-int arithmetic.  Measured on the development machine, one closed form and one witness map take

    L    Groth16 closed form   witness map   GM17 closed form
    12        0.76 s              0.39 s          1.46 s
    13        1.47 s              0.85 s          2.89 s
    14        2.88 s              1.82 s          5.75 s
    15        4.74 s              2.40 s         10.19 s
    16        9.56 s              6.33 s         18.73 s

A rung needs three closed forms (the batch of three over two assignments) and, for Groth16, two witness maps: 6 s of reference at
L = 13 for Groth16 and 9 s for GM17, 12 s and 17 s at L = 14.  The top rung of that curve is therefore L = 13, where the reference of
a CASE (not of a single proof: that would be L = 16 and a case of 40 s) stays at about ten seconds; the two schemes are cases of
their own."""
import json
import os
import subprocess

import pytest

import size_ladder as sl
from zokrates_amd import native

from emu_util import emu_library

NAMES = {0: "bn254", 1: "bls12_381", 2: "bls12_377"}
# the emulator half: the top rungs up to which a case stays cheap on fibres (the device-side setup of a BLS12-381 or BLS12-377 rung is
# 7 - 10 s there whatever its size; a BN254 rung 2 - 5 s).  Proofs: {curve: top L}, GM17 one rung below
EMU_NTT_MAX, EMU_NTT_377_MAX, EMU_PROOF_MAX, EMU_PROOF_377_MAX, EMU_ADHOC_MAX_N = 11, 9, {0: 5, 1: 1}, 1, 2048


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0, emu_library())
    assert "EMULATOR" in c.describe()
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu_ctx():
    c = native.Context(0)
    assert "gfx950" in c.describe() and "EMULATOR" not in c.describe()
    yield c
    c.close()


def emu_context():
    return native.Context(0, emu_library())


def gpu_context():
    c = native.Context(0)
    assert "EMULATOR" not in c.describe()
    return c


def ids():
    return lambda v: "%s%s" % (NAMES[v[0]], "".join("-%s" % x for x in v[1:])) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------ (a) coverage, on the model alone
def test_the_ladder_covers_every_shape():
    cov = sl.coverage()
    # table mode.  BN254: every width has its own window count, so 2 ... 17 are all chosen; the h launch reaches every one.  The
    # fused z launch and the G2 launch run over m + 2 entries and m + 2 >= 5 for any system with a constraint, so their narrowest
    # automatic width is 3: width 2 is reached by test_*_two_bit_windows_over_a_key under msm_c
    every = lambda cid: {sl.table_window(1 << k, sl.BITS[cid]) for k in range(1, 24)}
    assert every(0) == set(range(2, 18)) and every(1) == set(range(2, 17)) and every(2) == set(range(2, 18))
    for cid in (0, 1):
        assert cov["table"][cid]["h"] == every(cid), (cid, cov["table"][cid]["h"])
        assert cov["table"][cid]["z"] == every(cid) - {2}, (cid, cov["table"][cid]["z"])
        assert sl.table_window(5, sl.BITS[cid]) == 3
    # BLS12-377: the rungs its Python reference affords
    assert cov["table"][2]["h"] == set(range(2, 2 + len(sl.PROOF_LS_377))) and cov["table"][2]["z"] == set(range(3, 2 + len(sl.PROOF_LS_377)))
    # both sides of the one-level / two-level placement (K = 2^(c-1) against 2^MSM_COARSE_BITS) and the two histogram halves at 17
    shapes = {c: sl.msm_shape(1 << (c - 1), 254, True) for c in cov["table"][0]["z"]}
    assert all(s["c"] == c for c, s in shapes.items())
    b = sl.MSM_COARSE_BITS
    assert not shapes[b]["two_level"] and shapes[b + 1]["two_level"] and shapes[17]["two_level"]
    assert shapes[16]["halves"] == 1 and shapes[17]["halves"] == 2
    assert (shapes[b]["Lw"], shapes[b]["H"]) == (128, 1) and (shapes[b + 1]["Lw"], shapes[b + 1]["H"]) == (256, 1) and shapes[b + 2]["H"] == 2
    # ad-hoc mode: every width 2 ... 16 runs; the ones the rule never picks (their top window would hold two or three bits) under msm_c
    for cid in (0, 1):
        assert set(cov["adhoc"][cid]) == set(sl.ADHOC_WIDTHS), cov["adhoc"][cid]
        for c, n, forced in sl.adhoc_cases(cid):
            if forced:
                assert c not in sl.adhoc_rungs(cid)
            else:
                assert sl.adhoc_window(n, sl.BITS[cid]) == c and (n == 1 or c == 2 or sl.adhoc_window(n - 1, sl.BITS[cid]) != c)
    assert {c for c, f in cov["adhoc"][0].items() if f} == {11, 12, 14} and {c for c, f in cov["adhoc"][1].items() if f} == {11, 12, 14, 15}
    # transforms: every sub-length 1 ... 11 as the cols pass and as the rows pass of a two-pass plan; single-pass and three-pass plans;
    # every workgroup size
    assert cov["cols"] == set(range(1, 12)) and cov["rows"] == set(range(1, 12))
    assert cov["passes"][1] == set(range(0, 11)) and set(range(11, 23)) <= cov["passes"][2] and cov["passes"][3]
    assert cov["threads"] == {64, 128, 256, 512}
    by_default = [sl.ntt_plan(lg) for lg in sl.NTT_LOGS]
    assert {p["log1"] for p in by_default if p["passes"] == 2} == set(range(5, 12)) and {p["log2"] for p in by_default if p["passes"] == 2} == set(range(6, 12))
    assert sl.ntt_plan(23)["passes"] == 3 and sl.ntt_plan(22)["passes"] == 2          # (2^23 ... 2^28: tests/test_gpu_large_domains.py)
    # GM17 runs wherever its domain fits
    assert [L for L in sl.PROOF_LS if sl.gm17_runs(L)] == list(range(1, 19))


def test_the_model_of_the_plan_geometry():
    """The geometry get_plan derives, at the sizes where it changes: the tile of 1024 elements, 64 to 512 work-items, LDS."""
    p = sl.ntt_plan(10)
    assert (p["log1"], p["log2"], p["R_rows"], p["threads_rows"]) == (0, 10, 1, 256)
    p = sl.ntt_plan(11)
    assert (p["log1"], p["log2"], p["C_cols"], p["R_rows"], p["threads_cols"], p["threads_rows"]) == (5, 6, 32, 16, 256, 256)
    p = sl.ntt_plan(18)
    assert (p["log1"], p["log2"], p["C_cols"], p["R_rows"], p["threads_cols"], p["threads_rows"]) == (9, 9, 2, 2, 256, 256)
    p = sl.ntt_plan(22)
    assert (p["log1"], p["log2"], p["C_cols"], p["R_rows"], p["threads_cols"], p["threads_rows"]) == (11, 11, 2, 1, 512, 512)
    assert p["smem_cols"] == 9 * 2 * (2048 + 64 + 1) * 4
    p = sl.ntt_plan(23)
    assert (p["log1"], p["log2"], p["log3"], p["split"]) == (7, 8, 8, 7 | (8 << 8))


def test_the_model_of_the_plan_geometry_against_the_library(tmp_path):
    """size_ladder.ntt_plan against the library's own arithmetic (csrc/ntt_geom.h, from which get_plan and every pass launcher take
    their numbers), key by key, at every domain size under every setting of ntt_max_sublog (2 .. 11), ntt_single_max_log (0 .. 11)
    and ntt_cols (1, 2).  tests/host/ntt_geom.cpp — a stand-alone program on the CPU, under ASan + UBSan — holds the header to the
    rules written out on their own and prints the plan of every case."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "ntt_geom")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_EMU", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(here, "..", "zokrates_amd", "csrc"),
                           os.path.join(here, "host", "ntt_geom.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 failures" in out.stderr, out.stderr
    seen = set()
    for line in out.stdout.splitlines():
        got = json.loads(line)
        case = (got.pop("single_max"), got.pop("sub"), got.pop("ccols"), got["logN"])
        seen.add(case)
        want = sl.ntt_plan(case[3], single_max=case[0], sub=case[1], ccols=case[2])
        assert sorted(got) == sorted(want), (case, sorted(got), sorted(want))
        for key in want:
            assert got[key] == want[key], (case, key, got[key], want[key])
    assert seen == {(sm, sub, cc, lg) for sub in range(2, 12) for lg in range(0, min(3 * sub, 47) + 1) for sm in range(0, 12) for cc in (1, 2)}


def test_the_model_of_the_msm_shape_against_the_library(tmp_path):
    """size_ladder.msm_shape against the library's own arithmetic (csrc/msm_geom.h, from which msm_prepare and msm_run_tables take
    every size, grid and stride), key by key: the scalar widths of the three curves, with and without tables, n = 1, 2, 3 and
    2^k - 1, 2^k, 2^k + 1 up to 2^26, no forced width and every forced one.  tests/host/msm_geom.cpp — a stand-alone program on the
    CPU, under ASan + UBSan — holds the header to the rules written out on their own (the sort, the accumulation and the fold under
    every knob, the choice of bucket sets against the two loops it replaced) and prints the shape of every case."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "msm_geom")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_EMU", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(here, "..", "zokrates_amd", "csrc"),
                           os.path.join(here, "host", "msm_geom.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 failures" in out.stderr, out.stderr
    seen = set()
    for line in out.stdout.splitlines():
        got = json.loads(line)
        case = (got.pop("n"), got.pop("bits"), got.pop("table"), got.pop("force_c"))
        seen.add(case)
        want = sl.msm_shape(case[0], case[1], case[2], force_c=case[3])
        assert sorted(got) == sorted(want), (case, sorted(got), sorted(want))
        for key in want:
            assert got[key] == want[key], (case, key, got[key], want[key])
    ns = {1, 2, 3} | {(1 << k) + d for k in range(2, 27) for d in (-1, 0, 1)}
    assert seen == {(n, bits, table, c) for n in ns for bits in sl.BITS.values() for table in (False, True) for c in [0] + list(range(2, 18))}
    assert "%d cases, 0 failures" % len(seen) in out.stderr, out.stderr


# ------------------------------------------------------------------ (b) transforms at every size
NTT_RUNGS = [(cid, lg) for cid in (0, 1) for lg in sl.NTT_LOGS] + [(2, lg) for lg in sl.NTT_LOGS_377]
NTT_TUNED = [(cid, name) for cid in (0, 1) for name in sl.NTT_TUNED]


@pytest.mark.parametrize("rung", [r for r in NTT_RUNGS if r[1] <= (EMU_NTT_377_MAX if r[0] == 2 else EMU_NTT_MAX)], ids=ids())
def test_ntt(ctx, rung):
    sl.check_ntt_rung(ctx, *rung)


@pytest.mark.parametrize("rung", NTT_TUNED, ids=ids())
def test_ntt_tuned_plans(rung):
    sl.check_ntt_tuned(emu_context, *rung)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", NTT_RUNGS, ids=ids())
def test_gpu_ntt(gpu_ctx, rung):
    sl.check_ntt_rung(gpu_ctx, *rung)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", NTT_TUNED, ids=ids())
def test_gpu_ntt_tuned_plans(rung):
    sl.check_ntt_tuned(gpu_context, *rung)


# ------------------------------------------------------------------ (c) witness map and proofs at every size
G16_RUNGS = sorted([(cid, L, "full") for cid in (0, 1) for L in sl.PROOF_LS] + [(cid, L, "half") for cid in (0, 1) for L in sl.PROOF_HALF_LS])
GM17_RUNGS = [r for r in G16_RUNGS if sl.gm17_runs(r[1], r[2] == "half")]


# (the half-empty shapes take the oracle's key and are cheap at 2^3 on every curve; bn254-8-half on the emulator too: c_z = 8 and c_h = 9, the two sides of the one-level / two-level placement, in seven seconds)
@pytest.mark.parametrize("rung", [r for r in G16_RUNGS if r[1] <= EMU_PROOF_MAX[r[0]] or r[1:] == (3, "half") or r == (0, 8, "half")], ids=ids())
def test_g16(ctx, rung):
    sl.check_g16(ctx, rung[0], rung[1], rung[2] == "half")


@pytest.mark.parametrize("rung", [r for r in GM17_RUNGS if r[1] <= EMU_PROOF_MAX[r[0]] - 1 or r[1:] == (3, "half")], ids=ids())
def test_gm17(ctx, rung):
    sl.check_gm17(ctx, rung[0], rung[1], rung[2] == "half")


@pytest.mark.parametrize("L", [L for L in sl.PROOF_LS_377 if L <= EMU_PROOF_377_MAX])
@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_bls12_377(ctx, scheme, L):
    sl.check_g16_377(ctx, L, scheme == "gm17")


def _two_bit_windows(make_ctx, curve_id):
    c2 = make_ctx()
    try:
        c2.tune("msm_c", 2)
        sl.check_g16(c2, curve_id, 3, force_c=2)
    finally:
        c2.close()


@pytest.mark.parametrize("curve_id", [0], ids=lambda c: NAMES[c])
def test_two_bit_windows_over_a_key(curve_id):
    """width 2 in the fused z launch and the G2 launch, which no key's size picks (m + 2 >= 5): msm_c on a context of the test's own"""
    _two_bit_windows(emu_context, curve_id)


def _odd_two_pass_split(make_ctx, curve_id):
    c2 = make_ctx()
    try:
        c2.tune("ntt_single_max_log", 1)
        assert sl.ntt_plan(3, single_max=1)["split"] == 1
        sl.check_g16(c2, curve_id, 3, half=True, plan=dict(single_max=1))
    finally:
        c2.close()


@pytest.mark.parametrize("curve_id", [0, 1], ids=lambda c: NAMES[c])
def test_odd_two_pass_split_over_a_key(curve_id):
    """2^3 as 2^1 x 2^2 under ntt_single_max_log = 1: the h table's order and the proofs over a domain whose two factors differ, at a
    size the emulator affords; the key's header names the split.  (On the device the default plans do this from 2^11 on: the `gpu`
    rungs g16[*-11-full], [*-13-full], ...)"""
    _odd_two_pass_split(emu_context, curve_id)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", G16_RUNGS, ids=ids())
def test_gpu_g16(gpu_ctx, rung):
    sl.check_g16(gpu_ctx, rung[0], rung[1], rung[2] == "half")


@pytest.mark.gpu
@pytest.mark.parametrize("rung", GM17_RUNGS, ids=ids())
def test_gpu_gm17(gpu_ctx, rung):
    sl.check_gm17(gpu_ctx, rung[0], rung[1], rung[2] == "half")


@pytest.mark.gpu
@pytest.mark.parametrize("L", sl.PROOF_LS_377)
@pytest.mark.parametrize("scheme", ["g16", "gm17"])
def test_gpu_bls12_377(gpu_ctx, scheme, L):
    sl.check_g16_377(gpu_ctx, L, scheme == "gm17")


@pytest.mark.gpu
@pytest.mark.parametrize("curve_id", [0, 1], ids=lambda c: NAMES[c])
def test_gpu_two_bit_windows_over_a_key(curve_id):
    _two_bit_windows(gpu_context, curve_id)


# ------------------------------------------------------------------ (d) ad-hoc MSM at every width
ADHOC = [(cid, "c%d" % c, "n%d" % n, "forced" if forced else "auto") for cid in (0, 1) for c, n, forced in sl.adhoc_cases(cid)]


def _adhoc(make_ctx, shared, rung):
    cid, c, n, forced = rung[0], int(rung[1][1:]), int(rung[2][1:]), rung[3] == "forced"
    if not forced:
        return sl.check_adhoc_msm(shared, cid, c, n)
    c2 = make_ctx()
    try:
        sl.check_adhoc_msm(c2, cid, c, n, forced=True)
    finally:
        c2.close()


@pytest.mark.parametrize("rung", [r for r in ADHOC if int(r[2][1:]) <= EMU_ADHOC_MAX_N], ids=ids())
def test_adhoc_msm(ctx, rung):
    _adhoc(emu_context, ctx, rung)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", ADHOC, ids=ids())
def test_gpu_adhoc_msm(gpu_ctx, rung):
    _adhoc(gpu_context, gpu_ctx, rung)
