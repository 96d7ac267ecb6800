"""The branches of the MSM's launch geometry (csrc/msm_geom.h) that no other test reaches on the device: ad-hoc zkhip_msm over G1
and G2 of BN254, 300 points with 0, 1 and r - 1 among the scalars, bit for bit against oracle.cpu.msm.

tests/host/msm_geom.cpp holds the arithmetic to its rules on the CPU; these cases run what it sizes.  Of the shapes the geometry
distinguishes, two are left to the tests that already run them on the device: K = 8 < 256 (msm_c 4: one-level placement, Lw = 8,
H = 1, the final scan at its floor of 64 work-items) is test_size_ladder.py::test_gpu_adhoc_msm[bn254-c4-*], G1 and G2; K = 256
(msm_c 9: two-level placement, one-workgroup scan, H = 1) is test_gpu_adhoc_msm[bn254-c9-*] for G1 and the proofs of
test_gpu_g16[bn254-8-*] (c_z = 8, c_h = 9) for G2.  Here:

  * msm_c 14 — W K = 19 x 8192 = 155 648 counters, more than SCAN_ONE_MAX: the three-kernel scan and k_msm_tile_offsets, H = 32 rows
    — under fold_hg 1, 32 and 256 (a column's rows in 1, 32 and — clamped to H — 32 shares; CW = 256, 8, 8 columns per workgroup),
    under fold_scan 0 (H = 32, Lw = 256: the double-and-add form where the scan form would run), heavy_runs 0, msm_lanes 1 (one
    slice: one work-item walks the whole list) and msm_min_slice 1.  No other test sets fold_hg; the size ladder runs this width
    for G1 alone, on the defaults;
  * msm_c 17 — K = 2^16: the sort's two histogram halves over ONE chunk (n < 2 kh), and 15 bucket sets of 2^16 keys through the
    three-kernel scan (a key's tables at this width have one set, 2^16 counters, and take the one-workgroup scan).

Every case runs on the emulator too (CPU suite) and on the device (`gpu`)."""
import numpy as np
import pytest

import size_ladder as sl
from oracle import cpu
from oracle.fields import BN254
from zokrates_amd import native

from emu_util import emu_library

N = 300
DEFAULTS = {"msm_c": 0, "fold_hg": 32, "fold_scan": 1, "heavy_runs": 1, "msm_lanes": 0, "msm_min_slice": 8}
CASES = {
    "c14-hg1": {"msm_c": 14, "fold_hg": 1},
    "c14-hg32": {"msm_c": 14, "fold_hg": 32},                 # (fold_scan 1, heavy_runs 1: the defaults)
    "c14-hg256": {"msm_c": 14, "fold_hg": 256},
    "c14-final-double-and-add": {"msm_c": 14, "fold_scan": 0},
    "c14-no-heavy-runs": {"msm_c": 14, "heavy_runs": 0},
    "c14-one-lane": {"msm_c": 14, "msm_lanes": 1},
    "c14-min-slice-1": {"msm_c": 14, "msm_min_slice": 1},
    "c17": {"msm_c": 17},
}


@pytest.fixture(scope="module")
def case():
    """(G1 bases, G2 bases, scalars, the oracle's two answers), made once"""
    from test_gpu_parity import _bases
    m, g1, g2 = _bases(BN254, N - 4, 0x6E0)
    assert m == N
    ks = sl.uniform_fr(BN254, N, 0x6E0).reshape(-1, 32)          # r - 1 at 0, N / 2 and N - 1, 0 at N / 4
    ks[N // 4 + 1] = 0
    ks[N // 4 + 1, 0] = 1
    vals = {int.from_bytes(k.tobytes(), "little") for k in ks}
    assert {0, 1, BN254.r - 1} <= vals
    ks = ks.reshape(-1)
    g1, g2 = np.array(g1), np.array(g2)
    return g1, g2, ks, cpu.msm(0, 1, g1, ks), cpu.msm(0, 2, g2, ks)


def _model(knobs):
    """what the case is there for, by the model of the shape"""
    s = sl.msm_shape(N, sl.BITS[0], False, force_c=knobs["msm_c"])
    nkeys = s["sets"] * s["K"]
    if knobs["msm_c"] == 14:
        assert (s["W"], s["K"], s["H"], s["Lw"], s["halves"], s["two_level"]) == (19, 8192, 32, 256, 1, True) and nkeys == 155648 > 1 << 17
    else:
        assert (s["W"], s["K"], s["H"], s["Lw"], s["halves"], s["two_level"]) == (15, 1 << 16, 256, 256, 2, True) and nkeys > 1 << 17
        assert N < 2 * sl.MSM_SORT_MAX_KH                          # one chunk per (window, half)


def _run(ctx, case, knobs):
    g1, g2, ks, want1, want2 = case
    _model(knobs)
    try:
        for name, value in knobs.items():
            ctx.tune(name, value)
        assert ctx.msm(0, 1, g1, ks) == want1, ("G1", knobs)
        assert ctx.msm(0, 2, g2, ks) == want2, ("G2", knobs)
    finally:
        for name, value in DEFAULTS.items():
            ctx.tune(name, value)


@pytest.fixture(scope="module")
def emu_ctx():
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


@pytest.mark.parametrize("name", list(CASES))
def test_msm_geometry(emu_ctx, case, name):
    _run(emu_ctx, case, CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_msm_geometry(gpu_ctx, case, name):
    _run(gpu_ctx, case, CASES[name])
