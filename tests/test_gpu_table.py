"""The per-diagonal band table the device builds (cpecan_build_diag_table, one thread per region, and
cpecan_build_diag_table_wave, one wave per region; cpk_table_gather.inl) against tests/table_model.py, entry by entry,
on the constructed inputs of tests/table_cases.py -- whose edges tests/test_table_cases_cpu.py asserts without a device.
The table is read back with cpecan_batch_table_fetch (api.Batch.table), which needs no debug mode: what is compared is
the table of the plan that runs.  Integers only: every comparison is exact.

These tests upload and fetch; they do not run a sweep (a table that is wrong never drives one).  The one exception is
test_the_pinned_table_gives_the_oracles_lists, which runs the mixed batch once its table has passed."""
import numpy as np
import pytest

import oracle_binding as ob
import table_cases as tc
import table_model as tm
from cpecan_amd import api
from parity import assert_pairs_match

pytestmark = pytest.mark.gpu

CASE_PLANS = [(c.name, plan) for c in tc.all_cases() for plan in c.plans]
SPLIT_CASES = [c.name for c in tc.all_cases() if c.name != "mixed"]


def _sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)


@pytest.fixture
def knobs(monkeypatch):
    """plan(name, **more): the environment of one launch plan and nothing else of the planning knobs."""
    def plan(name, **more):
        for k in tc.OTHER_KNOBS + tuple(k for env in tc.PLANS.values() for k in env):
            monkeypatch.delenv(k, raising=False)
        for k, v in dict(tc.PLANS[name], **more).items():
            monkeypatch.setenv(k, v)
    return plan


def _uploaded(case, runs=False, debug=False):
    b = api.Batch(_sm(case.mtype), api.pairwiseAlignmentBandingParameters_construct(**case.pkw), debug=debug)
    (b.add_many_runs if runs else b.add_many)(case.problems)
    b.upload()
    return b


def _tables(b, case):
    """[(problem, region, table)] of every region of the batch."""
    out = []
    for i in range(len(case.problems)):
        first = b.table(i, 0)
        out.append((i, 0, first))
        out += [(i, r, b.table(i, r)) for r in range(1, first["nRegions"])]
    return out


def _fetch(case, **kw):
    with _uploaded(case, **kw) as b:
        return _tables(b, case)


def _errors(case, tables):
    model = tc.regions(case.name)
    assert [(i, r) for i, r, _ in tables] == [(i, r) for i, regs in enumerate(model) for r in range(len(regs))]
    return ["%s problem %d region %d (%s): %s" % (case.name, i, r, "split" if t["split"] else "whole", e)
            for i, r, t in tables for e in tm.check_region(model[i][r], t)]


def _same_words(name, got, want):
    """Two fetches of the same batch, word for word; the first differing diagonal and field otherwise."""
    assert len(got) == len(want)
    for (i, r, a), (_, _, b) in zip(got, want):
        where = "%s problem %d region %d: " % (name, i, r)
        assert a["split"] == b["split"] and a["ringCap"] == b["ringCap"], where + "planned differently"
        diff = tm.first_difference(a["diags"], b["diags"])
        assert diff is None, where + diff
        assert (a["dpos"] is None) == (b["dpos"] is None), where + "position words in one batch only"
        if a["dpos"] is not None:
            bad = np.flatnonzero(a["dpos"] != b["dpos"])
            assert len(bad) == 0, where + "diagonal %d dpos: got %#x, want %#x" % (bad[0], a["dpos"][bad[0]] & 0xffffffff,
                                                                                  b["dpos"][bad[0]] & 0xffffffff)


@pytest.mark.parametrize("name,plan", CASE_PLANS)
def test_table_equals_the_model(name, plan, knobs):
    """Every region of every case under every plan it was built for: xmyL, width and cellOff are the oracle band's,
    ringOff follows the rule of its ring (and, whole regions, keeps every segment's live diagonals apart), the position
    words keep their contract, and the region is planned as the model plans it."""
    case = tc.case(name)
    knobs(plan)
    tables = _fetch(case)
    errs = _errors(case, tables)
    assert not errs, "\n".join(errs[:12])
    with_segments = [t for _, _, t in tables if t["nSeg"] > 0]
    if plan in tc.SPLIT_PLANS:  # the forms the plan is named for really ran
        assert all(t["split"] for t in with_segments), name
        if case.positions:
            assert all(t["dpos"] is not None for _, _, t in tables), name
    elif plan == "whole":
        assert not any(t["split"] for _, _, t in tables) and all(t["dpos"] is None for _, _, t in tables), name
    else:
        assert any(t["split"] for _, _, t in tables) and any(not t["split"] for t in with_segments), name


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_wave_and_serial_builders_write_the_same_words(name, knobs):
    """One wave per region (the default for split regions) and one thread per region (CPECAN_TABLE_WAVE=0) build the same
    table and the same position words, in both split forms."""
    case = tc.case(name)
    for plan in tc.SPLIT_PLANS:
        knobs(plan)
        wave = _fetch(case)
        knobs(plan, CPECAN_TABLE_WAVE="0")
        serial = _fetch(case)
        assert any(t["split"] for _, _, t in wave), (name, plan)
        _same_words("%s %s wave against serial" % (name, plan), wave, serial)
        errs = _errors(case, serial)
        assert not errs, "\n".join(errs[:12])


@pytest.mark.parametrize("E", tc.RUN_EXPANSIONS)
@pytest.mark.parametrize("plan", ["whole", "split1"])
def test_runs_and_expanded_anchors_give_one_table(E, plan, knobs):
    """The same anchors as runs (cpecan_batch_add_many_runs: expanded on the device by cpecan_expand_runs), as runs
    expanded on the host (CPECAN_KEEP_RUNS=0) and as anchors (cpecan_batch_add_many)."""
    case = tc.case("runs-E%d" % E)
    knobs(plan)
    anchors = _fetch(case)
    kept = _fetch(case, runs=True)
    knobs(plan, CPECAN_KEEP_RUNS="0")
    expanded = _fetch(case, runs=True)
    _same_words("%s %s runs against anchors" % (case.name, plan), kept, anchors)
    _same_words("%s %s runs expanded on the host against anchors" % (case.name, plan), expanded, anchors)
    errs = _errors(case, kept)
    assert not errs, "\n".join(errs[:12])


def test_fetch_needs_an_upload_and_nothing_else(knobs):
    """CPECAN_ESTATE before upload, CPECAN_EINVAL for indices out of range; the same table with and without debug
    buffers wherever the two batches are planned alike (a debug batch is never packed), and position words only where the
    batch has them."""
    case = tc.case("multi-region")
    knobs("split1")
    with api.Batch(_sm(0), api.pairwiseAlignmentBandingParameters_construct(**case.pkw)) as b:
        b.add_many(case.problems)
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            b.table(0)
        b.upload()
        n = b.table(0)["nRegions"]
        assert n == len(tc.regions(case.name)[0]) >= 3
        for problem, region in ((-1, 0), (len(case.problems), 0), (0, -1), (0, n)):
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                b.table(problem, region)
        plain = _tables(b, case)
    _same_words("multi-region with debug buffers", _fetch(case, debug=True), plain)
    dynamic = tc.case("dynamic")
    assert all(t["dpos"] is None for _, _, t in _fetch(dynamic))  # per-anchor expansions: no position words are written


def test_the_pinned_table_gives_the_oracles_lists(knobs):
    """The one test that runs: the mixed batch (packed, wide and split classes side by side), its table checked first,
    then every problem's list against the oracle's -- and the table is the same after the run."""
    case = tc.case("mixed")
    knobs("mixed")
    with _uploaded(case) as b:
        before = _tables(b, case)
        errs = _errors(case, before)
        assert not errs, "\n".join(errs[:12])
        b.run()
        b.download()
        got = [b.result(i) for i in range(len(case.problems))]
        _same_words("mixed after the run", _tables(b, case), before)
    om, op = ob.model(case.mtype), ob.params(**case.pkw)
    for i, (sx, sy, a, rl, rr) in enumerate(case.problems):
        assert_pairs_match(got[i], ob.aligned_pairs(om, sx, sy, a, op, rl, rr), threshold=op.threshold)
