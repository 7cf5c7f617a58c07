"""Chains in the launch plan (cpk_plan.inl, plan_chains) without a GPU: the traceback launch of a two-launch class takes over
the forward sweep of every region's later segments -- one chain item per region with more than K segments -- where both
launches are gangs and the forward launch runs in rounds.  cpk_batch_launch_plan keeps its record; cpk_batch_chain_plan,
beside it, answers K and the number of chains per class and the traceback queues built from the plan."""
import ctypes as C

import pytest

from cpecan_amd import api
from cpecan_amd.workload import CONFIGS, config_problems, make_pair
from test_gang_plan_cpu import CUS, FIELDS, KNOBS, plan

SHORT = dict(minDiagsBetweenTraceBack=50, traceBackDiagonals=7)
ITEM_FIELDS = ("cls", "region", "seg", "cost", "nSeg", "fwdSegs")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS + ("CPECAN_CHAIN",):
        monkeypatch.delenv(k, raising=False)


def chain_plan(problems, mtype=0, max_items=1 << 17, **pkw):
    """([(K, chains)] per launch class, [item records in queue order]) of the plan for a device of 256 CUs that is not there."""
    f = api.lib().cpk_batch_chain_plan
    f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    f.restype = C.c_int
    chains = (C.c_int64 * (2 * 16))()
    items = (C.c_int64 * (len(ITEM_FIELDS) * max_items))()
    n_items = C.c_int64(0)
    sm = api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)
    with api.Batch(sm, api.pairwiseAlignmentBandingParameters_construct(**pkw)) as b:
        b.add_many(problems)
        n = f(b._h, CUS, 288 << 30, chains, 16, items, max_items, C.byref(n_items))
        assert n >= 0, api.lib().cpecan_last_error()
    assert n_items.value <= max_items
    recs = [dict(zip(ITEM_FIELDS, items[i * len(ITEM_FIELDS):(i + 1) * len(ITEM_FIELDS)])) for i in range(n_items.value)]
    return [(chains[2 * i], chains[2 * i + 1]) for i in range(n)], recs


@pytest.fixture(scope="module")
def config_b():
    cfg = CONFIGS["B"]
    return config_problems("B", range(cfg["n_pairs"]))


def _rule_holds(items, waves_trace):
    """The plan's cost rule on a queue with chains: ceil(chains / waves) x longest chain <= all cost / waves."""
    chain_costs = [it["cost"] for it in items if it["seg"] < 0]
    total = sum(it["cost"] for it in items)
    return bool(chain_costs) and -(-len(chain_costs) // waves_trace) * max(chain_costs) * waves_trace <= total


def test_config_b_takes_one_chain_per_region_and_keeps_every_other_number(config_b, monkeypatch):
    monkeypatch.setenv("CPECAN_CHAIN", "0")
    (before,) = plan(config_b, diagonalExpansion=100)
    ((k0, n0),), items0 = chain_plan(config_b, diagonalExpansion=100)
    assert (k0, n0) == (0, 0) and all(it["seg"] >= 0 for it in items0)
    assert before["items"] == len(items0) == sum(it["nSeg"] for it in items0 if it["seg"] == 0)  # today's plan: an item per segment
    assert (before["waves"], before["wavesTrace"], before["firstGrid"], before["gangWaves"], before["gangWavesTrace"]) == (2508, 11 * CUS, 228, 11, 11)
    monkeypatch.delenv("CPECAN_CHAIN")
    (c,) = plan(config_b, diagonalExpansion=100)
    # (the record's `items` counts traceback segments, a chain as those it covers -- cpecan_internal.h --: not even that moves;
    # the queue itself, which cpk_batch_chain_plan answers, is shorter)
    assert len(FIELDS) == 25 and {k for k in FIELDS if c[k] != before[k]} <= {"items"}
    ((K, chains),), items = chain_plan(config_b, diagonalExpansion=100)
    assert chains == c["regions"] == 10000 and K >= 1
    assert c["items"] == sum(it["nSeg"] - K if it["seg"] < 0 else 1 for it in items), "the record's items: the segments the queue hands out"
    assert len(items) == before["items"] - sum(it["nSeg"] - K for it in items if it["seg"] < 0) + chains < before["items"]
    # K is the smallest value the cost rule accepts: it holds on the plan's own queue and on no forced queue below it
    assert all(it["seg"] == -K for it in items if it["seg"] < 0) and _rule_holds(items, c["wavesTrace"])
    for k in range(1, K):
        monkeypatch.setenv("CPECAN_CHAIN", str(k))
        ((kf, _),), forced = chain_plan(config_b, diagonalExpansion=100)
        assert kf == k and not _rule_holds(forced, c["wavesTrace"])


def _same_with_and_without(problems, monkeypatch, **kw):
    default = plan(problems, **kw)
    chains, items = chain_plan(problems, **kw)
    assert all(kc == (0, 0) for kc in chains) and all(it["seg"] >= 0 for it in items), chains
    monkeypatch.setenv("CPECAN_CHAIN", "0")
    assert plan(problems, **kw) == default
    monkeypatch.delenv("CPECAN_CHAIN")
    return default


def test_config_a_plans_no_chains(monkeypatch):
    cfg = CONFIGS["A"]
    (c,) = _same_with_and_without(config_problems("A", range(cfg["n_pairs"])), monkeypatch, mtype=2, diagonalExpansion=cfg["expansion"])
    assert (c["gangWaves"], c["gangWavesTrace"], c["items"]) == (0, 0, 3000)


def test_a_shard_in_the_one_launch_form_plans_no_chains(config_b, monkeypatch):
    (c,) = _same_with_and_without(config_b[:1250], monkeypatch, diagonalExpansion=100)
    assert c["mode"] == 3 and c["regions"] == 1250  # kModeFused


def test_without_gangs_there_are_no_chains(config_b, monkeypatch):
    monkeypatch.setenv("CPECAN_GANG", "0")
    (c,) = _same_with_and_without(config_b, monkeypatch, diagonalExpansion=100)
    assert (c["gangWaves"], c["gangWavesTrace"], c["waves"]) == (0, 0, 2500)


def test_chain_0_is_todays_plan(config_b, monkeypatch):
    monkeypatch.setenv("CPECAN_CHAIN", "0")
    (c,) = plan(config_b, diagonalExpansion=100)
    chains, items = chain_plan(config_b, diagonalExpansion=100)
    assert chains == [(0, 0)] and c["items"] == len(items) and all(it["seg"] >= 0 for it in items)


def test_the_chain_builds_of_the_kernel_table_are_the_ones_the_gpu_tests_run(monkeypatch):
    """cpk_kernel_table_forms shows a CHAIN build as the gang it stands in for; cpk_kernel_table_chain, in step with it, tells
    them apart.  The CHAIN builds are the forward and the traceback gang of both state counts and nothing else, and a class
    with chains under the knobs of tests/test_gpu_trace_chains.py plans exactly those."""
    import match_cases as mc
    f = api.lib().cpk_kernel_table_chain
    f.argtypes = [C.POINTER(C.c_int64), C.c_int]
    f.restype = C.c_int
    flags = (C.c_int64 * 1024)()
    table = mc.kernel_table()
    assert f(flags, 1024) == len(table)
    built = [k for k, chain in zip(table, flags) if chain]
    assert all(k["family"] == mc.FAMILY_SWEEP and k["emit"] == mc.EMIT_MATCH and k["gang"] and k["abs"] and k["wps"] == 3 for k in built)
    for name, v in (("CPECAN_PACKED", "0"), ("CPECAN_SPLIT", "1"), ("CPECAN_GANG", "2"), ("CPECAN_CHAIN", "1")):
        monkeypatch.setenv(name, v)
    planned = set()
    for mtype in (0, 2):
        (c,) = plan(mixed_problems(), mtype=mtype, **MIXED_PKW)
        ((K, chains),), _ = chain_plan(mixed_problems(), mtype=mtype, **MIXED_PKW)
        assert K == 1 and chains > 0 and (c["gangWaves"], c["gangWavesTrace"]) == (2, 2)
        planned |= {(c["nStates"], c["mode"]), (c["nStates"], mc.MODE_TRACE)}
    assert sorted((k["S"], k["mode"]) for k in built) == sorted(planned) == [(3, 1), (3, 2), (5, 1), (5, 2)]


# ---- coverage: regions of 1, 2, 3 and many segments in one class ----
def mixed_problems():
    """Anchored pairs of 20 to 320 bases under an expansion of 10: a segment every ~50 diagonals of a narrow band."""
    return [make_pair(31, i, length, 10) for i, length in enumerate((20, 45, 70, 320, 22, 48, 75, 260, 330))]


MIXED_PKW = dict(diagonalExpansion=10, **SHORT)


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_every_segment_is_swept_and_traced_exactly_once(k, monkeypatch):
    for name, v in (("CPECAN_PACKED", "0"), ("CPECAN_SPLIT", "1"), ("CPECAN_GANG", "2"), ("CPECAN_CHAIN", str(k))):
        monkeypatch.setenv(name, v)
    chains, items = chain_plan(mixed_problems(), **MIXED_PKW)
    assert len(chains) == 1, "one class"
    n_seg = {}
    for it in items:
        n_seg.setdefault(it["region"], it["nSeg"])
        assert n_seg[it["region"]] == it["nSeg"]
    assert len(n_seg) == len(mixed_problems())
    assert {1, 2, 3} <= set(n_seg.values()) and max(n_seg.values()) >= 8, sorted(n_seg.values())
    assert chains[0] == (k, sum(1 for n in n_seg.values() if n > k))
    for region, n in n_seg.items():
        mine = [it["seg"] for it in items if it["region"] == region]
        (fwd,) = {it["fwdSegs"] for it in items if it["region"] == region}  # where the library says the forward launch stops
        assert fwd == (n if n <= k else k)  # behind k segments of a longer region
        by_forward_launch = set(range(fwd))
        by_chain = set(range(k, n)) if -k in mine else set()
        assert sorted(by_forward_launch | by_chain) == list(range(n)) and not (by_forward_launch & by_chain)
        assert (-k in mine) == (n > k) and mine.count(-k) <= 1
        traced = sorted([s for s in mine if s >= 0] + sorted(by_chain))
        assert traced == list(range(n)), (region, mine)
    costs = [it["cost"] for it in items]
    assert costs == sorted(costs, reverse=True) and min(costs) > 0


def test_the_turn_back_shapes_move_the_base_on_both_diagonals_of_a_resume_point():
    """tests/test_gpu_trace_chains.py runs table_cases.chain_case with chains from segments 1, 2 and 4: in problem 0 the base
    must move in front of the top diagonal of segments 0 and 3, in problem 1 in front of the diagonal behind the top of
    segment 1 -- the diagonals a chain puts back from the ring and the first one it computes."""
    import table_cases as tc
    import table_model as tm
    case = tc.chain_case()
    hits = set()
    for pi, prob in enumerate(case.problems[:2]):
        (rg,) = tm.problem_regions(prob, case.pkw)
        danger = set(tm.danger_diagonals(rg.lo, rg.width))
        for si, (_, top, _) in enumerate(rg.segs[:-1]):
            hits |= {(pi, si + 1, "dTop")} if top in danger else set()
            hits |= {(pi, si + 1, "dTop+1")} if top + 1 in danger else set()
    assert {(0, 1, "dTop"), (0, 4, "dTop"), (1, 2, "dTop+1")} <= hits, sorted(hits)
