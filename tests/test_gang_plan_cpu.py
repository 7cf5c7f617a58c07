"""The launch plan's gangs (cpk_plan.inl: workgroups of several waves that share one copy of the LDS tables) without a GPU:
cpk_batch_launch_plan plans an unfrozen batch for a device of 256 CUs that is not there -- a kernel is taken to use the
registers its build allows -- and returns the numbers of every launch class."""
import ctypes as C

import pytest

from cpecan_amd import api
from cpecan_amd.workload import CONFIGS, config_problems, make_batch, make_pair

FIELDS = ("packed", "k", "regions", "maxWidth", "nStates", "family", "mode", "wps", "abs", "gang", "traceWps", "traceGang", "waves",
          "wavesTrace", "gangWaves", "gangWavesTrace", "ldsBytes", "ldsBytesFwd", "firstLdsBytes", "traceLdsBytes", "subSlots",
          "threads", "items", "firstGrid", "globalRows")
CUS = 256
CU_LDS = 160 * 1024
TABLES = 8 * (64 + 168)  # logAdd cubics + (emission + transition) sums: what a gang keeps once
MODE_FORWARD = 1
KNOBS = ("CPECAN_GANG", "CPECAN_SPLIT", "CPECAN_ABS", "CPECAN_ABS_WINDOWS", "CPECAN_PACKED", "CPECAN_MAX_WAVES_PER_CU", "CPECAN_TRACE3",
         "CPECAN_FWD3", "CPECAN_DENSE", "CPECAN_TEAM", "CPECAN_MEM_BUDGET_MB", "CPECAN_SPLIT_BUDGET_FRAC")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def plan(problems, mtype=0, **pkw):
    f = api.lib().cpk_batch_launch_plan
    f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.c_int]
    f.restype = C.c_int
    out = (C.c_int64 * (len(FIELDS) * 16))()
    sm = api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)
    with api.Batch(sm, api.pairwiseAlignmentBandingParameters_construct(**pkw)) as b:
        b.add_many(problems)
        n = f(b._h, CUS, 288 << 30, out, 16)
        assert n >= 0, api.lib().cpecan_last_error()
    return [dict(zip(FIELDS, out[i * len(FIELDS):(i + 1) * len(FIELDS)])) for i in range(n)]


@pytest.fixture(scope="module")
def config_b():
    """BASELINE config B: 10 000 pairs of 2 kb, five states, expansion 100."""
    cfg = CONFIGS["B"]
    assert (cfg["n_pairs"], cfg["length"], cfg["expansion"], cfg["model"]) == (10000, 2000, 100, "fiveState")
    return config_problems("B", range(cfg["n_pairs"]))


def _within_a_cu(classes):
    for c in classes:
        assert c["firstLdsBytes"] <= CU_LDS and c["traceLdsBytes"] <= CU_LDS, c
        assert c["gangWaves"] <= 12 and c["gangWavesTrace"] <= 12, c
        assert (c["gangWaves"] > 1) == bool(c["gang"]) and (c["gangWavesTrace"] > 1) == bool(c["traceGang"]), c
        if c["gangWaves"] > 1:  # whole gangs, the tables once
            assert c["waves"] % c["gangWaves"] == 0 and c["firstGrid"] * c["gangWaves"] == c["waves"], c
            assert c["firstLdsBytes"] == TABLES + c["gangWaves"] * (c["ldsBytesFwd"] - TABLES), c
        if c["gangWavesTrace"] > 1:
            assert c["wavesTrace"] % c["gangWavesTrace"] == 0 and c["subSlots"] >= c["wavesTrace"], c
            assert c["traceLdsBytes"] == TABLES + c["gangWavesTrace"] * (c["ldsBytes"] - TABLES), c


def test_config_b_items_run_as_one_gang_of_eleven_per_cu(config_b):
    (c,) = plan(config_b, diagonalExpansion=100)
    assert (c["regions"], c["maxWidth"], c["nStates"], c["mode"], c["abs"]) == (10000, 157, 5, MODE_FORWARD, 1)
    assert (c["ldsBytes"], c["ldsBytesFwd"]) == (16064, 15552)
    # the traceback launch: eleven waves per CU as one workgroup of 11 x (16 064 - 1 856) + 1 856 bytes
    assert (c["gangWavesTrace"], c["traceLdsBytes"], c["wavesTrace"], c["traceWps"]) == (11, 158144, 11 * CUS, 3)
    assert c["subSlots"] >= 11 * CUS
    # the forward launch keeps its four rounds -- eleven waves per CU do not take one off -- and the 2500 waves that the
    # rounds, evened out, ask for: laid out as 228 whole gangs of 11 x (15 552 - 1 856) + 1 856 bytes, all resident at once
    assert -(-10000 // c["waves"]) == 4 and 2500 <= c["waves"] < 2500 + 11
    assert (c["gangWaves"], c["waves"], c["firstGrid"], c["firstLdsBytes"], c["wps"]) == (11, 2508, 228, 152512, 3)
    assert c["firstGrid"] <= CUS
    _within_a_cu([c])


def test_gang_0_is_the_plan_without_gangs(config_b, monkeypatch):
    """CPECAN_GANG=0: config B as it was planned before there were gangs -- ten single-wave workgroups per CU for the items,
    2500 waves in four rounds for the regions --, and everything but the waves and the LDS of the two launches is what the
    default plans."""
    default = plan(config_b, diagonalExpansion=100)[0]
    monkeypatch.setenv("CPECAN_GANG", "0")
    (c,) = plan(config_b, diagonalExpansion=100)
    assert (c["waves"], c["wavesTrace"], c["subSlots"], c["ldsBytes"], c["ldsBytesFwd"], c["firstLdsBytes"], c["traceLdsBytes"]) == \
        (2500, 10 * CUS, 10 * CUS, 16064, 15552, 15552, 16064)
    assert (c["gang"], c["traceGang"], c["gangWaves"], c["gangWavesTrace"], c["wps"], c["traceWps"], c["threads"]) == (0, 0, 0, 0, 3, 3, 64)
    changed = {k for k in FIELDS if c[k] != default[k]}
    assert changed == {"gang", "waves", "gangWaves", "firstLdsBytes", "firstGrid",
                       "traceGang", "wavesTrace", "gangWavesTrace", "traceLdsBytes", "subSlots"}, changed


def test_a_queue_that_does_not_fill_the_gangs_keeps_single_waves():
    """BASELINE config A: 1000 regions and 3000 items for 3072 gang slots, kernels for two waves per SIMD in the traceback
    launch: gangs would crowd the waves onto a third of the CUs.  The plan is the one without gangs."""
    cfg = CONFIGS["A"]
    (c,) = plan(config_problems("A", range(cfg["n_pairs"])), mtype=2, diagonalExpansion=cfg["expansion"])
    assert (c["regions"], c["items"], c["mode"], c["abs"]) == (1000, 3000, MODE_FORWARD, 1)
    assert (c["gangWaves"], c["gangWavesTrace"], c["waves"], c["wavesTrace"], c["firstGrid"]) == (0, 0, 1000, 8 * CUS, 1000)


def test_forced_sizes(config_b, monkeypatch):
    """CPECAN_GANG=n: n waves per workgroup in both launches, as many workgroups per CU as fit; 10 is one gang of ten."""
    for n, per_cu in ((2, 10), (3, 9), (5, 10), (10, 10), (11, 11), (12, 0)):
        monkeypatch.setenv("CPECAN_GANG", str(n))
        (c,) = plan(config_b, diagonalExpansion=100)
        _within_a_cu([c])
        if per_cu == 0:  # twelve do not fit: no gang
            assert (c["gangWaves"], c["gangWavesTrace"], c["wavesTrace"]) == (0, 0, 10 * CUS)
            continue
        assert (c["gangWaves"], c["gangWavesTrace"]) == (n, n)
        assert c["wavesTrace"] == per_cu * CUS
        assert 2500 <= c["waves"] < 2500 + n  # the regions keep their four rounds


def test_room_for_no_wave_more_plans_no_gang(monkeypatch):
    """Unanchored 1050 x 1050 pairs, three states: rows of ~1050 cells, over 50 KB per wave -- close to the 64 KiB at which
    the LDS path ends, so a private block never leaves room for one wave only.  As many waves fit on a CU with the tables
    in each as with the tables shared: the wave more that a gang is taken for is not there, so the plan takes none."""
    monkeypatch.setenv("CPECAN_SPLIT", "1")
    monkeypatch.setenv("CPECAN_TEAM", "0")
    sx, sy, _ = make_pair(5, 0, 1050, 0)
    pkw = dict(minDiagsBetweenTraceBack=400, traceBackDiagonals=40)
    (c,) = plan([(sx, sy, ())] * 3, mtype=2, **pkw)
    assert (c["abs"], c["mode"], c["maxWidth"]) == (1, MODE_FORWARD, 1051) and c["ldsBytes"] > 50000, c
    per_cu = CU_LDS // c["ldsBytes"]
    assert (CU_LDS - TABLES) // (c["ldsBytes"] - TABLES) == per_cu, c
    assert c["gangWaves"] == 0 and c["gangWavesTrace"] == 0, c
    monkeypatch.setenv("CPECAN_GANG", str(per_cu + 1))  # ... and one more does not fit: forcing it changes nothing
    (forced,) = plan([(sx, sy, ())] * 3, mtype=2, **pkw)
    assert forced == c


@pytest.mark.parametrize("gang", [None, "2", "3", "7", "11", "12"])
def test_no_plan_exceeds_a_cu(gang, monkeypatch):
    """Bands of 9 to ~330 cells, both state counts, forced split: no workgroup declares more than 163 840 B or has more than
    twelve waves."""
    if gang:
        monkeypatch.setenv("CPECAN_GANG", gang)
    monkeypatch.setenv("CPECAN_SPLIT", "1")
    monkeypatch.setenv("CPECAN_PACKED", "0")
    seen = 0
    for mtype in (0, 2):
        for length, e in ((300, 4), (600, 20), (1000, 50), (2000, 100), (1500, 160), (1200, 240)):
            classes = plan(make_batch(7, 5, length, e), mtype=mtype, diagonalExpansion=e)
            _within_a_cu(classes)
            seen += sum(1 for c in classes if c["gangWavesTrace"] > 1)
    assert seen > 0 or gang is None  # (five pairs do not fill the gangs: unforced, these batches plan none)
