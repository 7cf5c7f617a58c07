"""The band-edge statistic on the device (cpecan_post_band_edge, cpk_post.inl; Batch.set_band_edge / Batch.band_edge)
against tests/band_edge_model.py and against the host's own statement of the definition (cpecan_band_edge_of_pairs), on
the constructed inputs of tests/band_edge_cases.py -- whose edges tests/test_band_edge_cpu.py asserts without a device.

The statistic is a pure integer function of the batch's own list 0 and its band, so every comparison is exact: the
model is applied to the lists of a twin batch without the switch and without consumers, and the lists of the batch with
the switch on are bit-equal to the twin's."""
import ctypes as C
import re
import sys

import numpy as np
import pytest

import band_edge_cases as bc
import band_edge_model as bm
from cpecan_amd import api

pytestmark = pytest.mark.gpu

ONE_WAVE, TEAM = "one wave per region", "a team of waves per region"
CASES = [c.name for c in bc.all_cases()]


@pytest.fixture
def knobs(monkeypatch):
    """env(**knobs): these planning knobs and no others; the host trace is on, so a test can see which kernel ran."""
    def env(**more):
        for k in bc.KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("CPECAN_TRACE_HOST", "1")
        for k, v in more.items():
            monkeypatch.setenv(k, v)
    return env


def _add(b, case):
    if not case.minus:
        b.add_many(case.problems)
        return
    # the caller of a minus problem holds the forward query: the batch makes the reverse complement it aligns
    arr, n, _keep = api.Batch.prepare_problems_runs([(sx, bc.reverse_complement(sy), a, rl, rr) for sx, sy, a, rl, rr in case.problems])
    minus = (C.c_int32 * n)(*([1] * n))
    api._check(api.lib().cpecan_batch_add_many_runs_stranded(b._h, arr, minus, n), "cpecan_batch_add_many_runs_stranded")
    assert all(b.problem_strand(i) == "minus" for i in range(n))


def _run(case, edge, post=None):
    """(list 0 per problem, statistic per problem or None, extra lists per problem, traceback segments of every problem's
    first region)."""
    sm = api.stateMachine5_construct(case.mtype)
    p = api.pairwiseAlignmentBandingParameters_construct(**case.pkw)
    with api.Batch(sm, p, emit=case.emit) as b:
        if post:
            b.set_post(*post)
        if edge:
            b.set_band_edge(True)
        _add(b, case)
        b.upload()
        b.run()
        b.download()
        n = len(case.problems)
        lists = [b.result(i) for i in range(n)]
        others = [[b.result(i, w) for w in ((1, 2) if case.emit == bc.EMIT_INDEL else ())] for i in range(n)]
        return lists, ([b.band_edge(i) for i in range(n)] if edge else None), others, [b.table(i)["nSeg"] for i in range(n)]


def _traced(case, capfd, edge, post=None):
    printed = capfd.readouterr().out
    out = _run(case, edge, post)
    err = capfd.readouterr().err
    sys.stdout.write(printed)
    return out + (err,)


def _expected(case, lists):
    """The model and the host function on the batch's own lists: they agree, and that is what the device must give."""
    want = []
    for pr, pairs in zip(case.problems, lists):
        model = bm.band_edge(pr, case.pkw, pairs)
        p = api.pairwiseAlignmentBandingParameters_construct(**case.pkw)
        assert api.band_edge_of_pairs(pr[2], len(pr[0]), len(pr[1]), p, pairs, pr[3], pr[4]) == model
        want.append(model)
    return want


def _check_flags(case, edges):
    for i, (e, claim) in enumerate(zip(edges, case.expect)):
        if claim == "flag":
            assert e["edgeScoreSum"] >= bc.S, (case.name, i, e)
        elif claim == "clear":
            assert e["edgeScoreSum"] < bc.S, (case.name, i, e)


def _kernel_ran(case, err):
    wide = re.findall(r"^cpecan class \d+:.*$", err, re.M)
    packed = re.findall(r"^cpecan packed class \d+:.*$", err, re.M)
    if case.env.get("CPECAN_PACKED") == "2":
        assert packed, err
    elif case.env.get("CPECAN_PACKED") == "0":
        assert wide and not packed and all(ONE_WAVE in c for c in wide), err
    elif "CPECAN_TEAM" in case.env:
        assert wide and all(TEAM in c for c in wide), err


@pytest.mark.parametrize("name", CASES)
def test_statistic_equals_the_model_on_the_batchs_own_lists(name, knobs, capfd):
    case = bc.case(name)
    knobs(**case.env)
    twin, _, twin_others, _, err = _traced(case, capfd, edge=False)
    _kernel_ran(case, err)
    lists, edges, others, segs, err = _traced(case, capfd, edge=True)
    _kernel_ran(case, err)
    for i in range(len(case.problems)):  # the switch changes no list
        assert lists[i].shape == twin[i].shape and (lists[i] == twin[i]).all(), (name, i)
        for a, b in zip(others[i], twin_others[i]):
            assert a.shape == b.shape and (a == b).all(), (name, i)
    want = _expected(case, twin)
    assert edges == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(edges, want)) if g != w][:3])
    _check_flags(case, edges)
    print(name, [(e["edgePairs"], e["edgeScoreSum"]) for e in edges])
    if name == "del400-chunks":  # several chunks per region: one per traceback segment that emitted a pair
        assert min(segs) > 10, segs


def test_consumers_do_not_change_the_statistic(knobs, capfd):
    """REWEIGHT | ORDERED, the realign flow's consumers: REWEIGHT rewrites the scores of list 0, and the statistic is still
    that of the scores the sweep emitted."""
    case = bc.case("del150-E4")
    knobs(**case.env)
    twin = _run(case, edge=False)[0]
    lists, edges = _run(case, edge=True, post=(api.POST_REWEIGHT | api.POST_ORDERED, 0.5, 0.85))[:2]
    assert edges == _expected(case, twin)
    assert any((a[:, 0] != b[:, 0]).any() for a, b in zip(lists, twin))  # the consumer did run
    assert all((a[:, 1:] == b[:, 1:]).all() for a, b in zip(lists, twin))
    indel = bc.case("indel")
    twin = _run(indel, edge=False)[0]
    edges = _run(indel, edge=True, post=(api.POST_MEA | api.POST_LEFT_SHIFT, 0.5))[1]
    assert edges == _expected(indel, twin)


FORMS = {
    "whole": {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "0"},
    "split1": {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "1"},
    "split2": {"CPECAN_PACKED": "0", "CPECAN_SPLIT": "2"},
    "packed": {"CPECAN_PACKED": "2"},
    "team": {"CPECAN_TEAM": "100"},
    "no-team": {"CPECAN_TEAM": "0"},
}


@pytest.mark.parametrize("name,forms", [("del150-E8", ("packed", "whole", "split1")), ("del400-chunks", ("whole", "split1", "split2", "packed")),
                                        ("two-regions", ("packed", "whole", "split1")), ("unanchored-team", ("team", "no-team")),
                                        ("del400-sweep", ("whole", "split1", "split2"))])
def test_every_launch_form_gives_the_same_statistic(name, forms, knobs):
    case = bc.case(name)
    seen = []
    for form in forms:
        knobs(**FORMS[form])
        lists, edges = _run(case, edge=True)[:2]
        assert edges == _expected(case, lists), (name, form)
        seen.append(edges)
    assert all(e == seen[0] for e in seen), (name, forms, seen)
    _check_flags(case, seen[0])


def test_the_switch_is_read_at_download(knobs):
    """CPECAN_ESTATE for a run that was not asked for the statistic; the switch set after a download takes effect at the
    next one, on the helper thread as well; problems without a pair read zeros."""
    knobs()
    case = bc.case("del150-E4")
    probs = list(case.problems[:4]) + [("", "ACGT", (), True, True), ("ACGT", "", (), False, False)]
    zero = {"edgePairs": 0, "edgeScoreSum": 0, "edgeScoreMax": 0}
    with api.Batch(api.stateMachine5_construct(), api.pairwiseAlignmentBandingParameters_construct(**case.pkw)) as b:
        b.add_many(probs)
        b.upload()
        b.run()
        b.download()
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            b.band_edge(0)
        first = [b.result(i) for i in range(len(probs))]
        b.set_band_edge(True)
        b.run()
        b.download()
        edges = [b.band_edge(i) for i in range(len(probs))]
        assert all((b.result(i) == first[i]).all() for i in range(len(probs)))
        assert edges[:4] == [bm.band_edge(pr, case.pkw, l) for pr, l in zip(probs[:4], first)] and edges[4:] == [zero, zero]
        assert edges[0]["edgePairs"] > 0
        for bad in (-1, len(probs)):
            with pytest.raises(api.CpecanError, match=r"\(-1\)"):
                b.band_edge(bad)
        b.run()
        b.download_begin()
        b.download_end()
        assert [b.band_edge(i) for i in range(len(probs))] == edges
        b.set_band_edge(False)
        b.run()
        b.download()
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            b.band_edge(0)
    with api.Batch(api.stateMachine5_construct()) as b:  # a batch without a problem
        b.set_band_edge(True)
