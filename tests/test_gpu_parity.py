"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same inputs.
Run on the MI355X box with `pytest -m gpu`."""
import random

import numpy as np
import pytest

import oracle_binding as ob
from cpecan_amd import api
from cpecan_amd.workload import make_batch, make_pair
from parity import assert_pairs_match, assert_log_close

pytestmark = pytest.mark.gpu

_ALPHABET = "AaCcGgTt" * 11 + "N"


def _rand_seq(rng, n):
    return "".join(rng.choice(_ALPHABET) for _ in range(n))


def _evolve(rng, s):
    s = "".join(rng.choice(_ALPHABET) if rng.random() > 0.8 else ch for ch in s)
    while rng.random() > 0.2:
        s = s.replace(_rand_seq(rng, rng.randrange(2, 4)), _rand_seq(rng, rng.randrange(0, 10)))
    return s


def _rand_anchors(rng, lX, lY):
    out, x, y = [], -1, -1
    while True:
        x += rng.randrange(1, 20)
        y += rng.randrange(1, 20)
        if x >= lX or y >= lY:
            return out
        out.append((x, y, 2 * rng.randrange(0, 5)))


def _sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype in (0, 1) else api.stateMachine3_construct(mtype)


def _run_batch(mtype, problems, raggeds=None, **pkw):
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
    with api.Batch(_sm(mtype), p) as b:
        for i, (sx, sy, a) in enumerate(problems):
            rl, rr = raggeds[i] if raggeds else (False, False)
            b.add(sx, sy, a, rl, rr)
        b.upload()
        b.run()
        b.download()
        return [b.result(i) for i in range(len(problems))], b.stats()


def _check_batch(mtype, problems, raggeds=None, **pkw):
    got, st = _run_batch(mtype, problems, raggeds, **pkw)
    om, op = ob.model(mtype), ob.params(**pkw)
    worst = 0.0
    for i, (sx, sy, a) in enumerate(problems):
        rl, rr = raggeds[i] if raggeds else (False, False)
        want = ob.aligned_pairs(om, sx, sy, a, op, rl, rr)
        worst = max(worst, assert_pairs_match(got[i], want, threshold=op.threshold))
    return worst, st


def test_known_answer_pairs():
    # tests/pairwiseAlignerTest.c:242-324 + SURVEY 8c scores
    p = api.pairwiseAlignmentBandingParameters_construct(threshold=0.2)
    got = api.getAlignedPairsUsingAnchors(api.stateMachine5_construct(), "AGCG", "AGTTCG", (), p)
    assert got.tolist() == [[9944673, 0, 0], [9259684, 1, 1], [8665179, 2, 4], [9893294, 3, 5]]


@pytest.mark.parametrize("mtype", [0, 2])
def test_config1_plumbing_full_dp(mtype):
    # BASELINE configs[0]: ~200 bp, no anchors -> full (unbanded) DP
    sx, sy, _ = make_pair(1, 0, 200, 0)
    _check_batch(mtype, [(sx, sy, ())])


def test_empty_and_degenerate_inputs():
    probs = [("", "", ()), ("ACGT", "", ()), ("", "ACGTN", ()), ("A", "A", ()), ("N", "T", ()), ("ACGTACGT", "ACG", ())]
    got, _ = _run_batch(0, probs)
    assert len(got[0]) == 0 and len(got[1]) == 0 and len(got[2]) == 0
    _check_batch(0, probs)
    _check_batch(2, probs)


def test_random_banded_property_like_reference():
    # tests/pairwiseAlignerTest.c:403-438: random anchors, random traceback parameters, random expansions
    rng = random.Random(21)
    for _ in range(25):
        sx = _rand_seq(rng, rng.randrange(0, 100))
        sy = _evolve(rng, sx)
        tbd = rng.randrange(1, 10)
        kw = dict(traceBackDiagonals=tbd, minDiagsBetweenTraceBack=tbd + rng.randrange(2, 10),
                  diagonalExpansion=2 * rng.randrange(0, 10), dynamicAnchorExpansion=int(rng.random() > 0.5),
                  splitMatrixBiggerThanThis=10 ** 12)
        _check_batch(0, [(sx, sy, _rand_anchors(rng, len(sx), len(sy)))], **kw)


def _fuzz_seeds(default):
    """CPECAN_FUZZ_SEEDS=lo:hi widens the fuzz tests for a soak run on the GPU box."""
    import os
    spec = os.environ.get("CPECAN_FUZZ_SEEDS")
    if not spec:
        return default
    lo, hi = (int(v) for v in spec.split(":"))
    return list(range(lo, hi))


@pytest.mark.parametrize("seed", _fuzz_seeds([101, 102, 103, 104]))
def test_fuzz_batches_all_paths(seed):
    """Random batches that mix everything a batch can hold: lengths 0-600, dense / sparse / no anchors (bands from a few
    cells to whole rectangles), ragged ends, splitting by large gaps, short and long traceback schedules, thresholds down
    to 0, all four model types -- so that packed classes, wide classes, multi-segment tracebacks and split regions meet
    in one launch.  Every problem against the oracle."""
    rng = random.Random(seed)
    for _ in range(3):
        mtype = rng.choice([0, 1, 2, 3])
        tbd = rng.choice([1, 3, 10, 40])
        pkw = dict(traceBackDiagonals=tbd, minDiagsBetweenTraceBack=tbd + rng.choice([2, 7, 60, 960]),
                   diagonalExpansion=2 * rng.choice([0, 2, 3, 5, 10, 20, 40]), threshold=rng.choice([0.0, 0.01, 0.2]),
                   splitMatrixBiggerThanThis=rng.choice([10, 900, 10 ** 12]),
                   dynamicAnchorExpansion=int(rng.random() < 0.3))  # then every anchor brings its own expansion
        probs, raggeds = [], []
        for _ in range(rng.randrange(30, 90)):
            sx = _rand_seq(rng, rng.choice([0, 1, 5, 40, 150, 300, 600]))
            sy = _evolve(rng, sx) if sx and rng.random() > 0.1 else _rand_seq(rng, rng.randrange(0, 80))
            kind = rng.random()
            anchors = []
            if kind < 0.6 and sx and sy:  # along the main diagonal, dense or sparse
                step = rng.choice([1, 7, 30, 120])
                x = y = rng.randrange(0, 5)
                while x < len(sx) and y < len(sy):
                    anchors.append((x, y, 2 * rng.randrange(0, 25) if pkw["dynamicAnchorExpansion"] else pkw["diagonalExpansion"]))
                    x += step + rng.randrange(0, 3)
                    y += step + rng.randrange(0, 3)
            elif kind < 0.8:
                anchors = [(x, y, e if pkw["dynamicAnchorExpansion"] else pkw["diagonalExpansion"])
                           for x, y, e in _rand_anchors(rng, len(sx), len(sy))]
            probs.append((sx, sy, anchors))
            raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
        if mtype in (1, 3):  # the asymmetric types only come from a loaded HMM (hmm_getStateMachine)
            ph, oh = api.hmm_constructEmpty(0.0, mtype), ob.hmm(mtype, 0.0)
            S = ph.stateNumber
            for i in range(S * S):
                ph.transitions[i] = oh.T[i] = 0.05 + rng.random()
            for i in range(S * 16):
                ph.emissions[i] = oh.E[i] = 0.05 + rng.random()
            api.hmm_normalise(ph)
            ob.lib().orc_hmm_normalise(oh)
            sm, om = api.hmm_getStateMachine(ph), ob.model_from_hmm(oh)
        else:
            sm, om = _sm(mtype), ob.model(mtype)
        p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
        op = ob.params(**pkw)
        with api.Batch(sm, p) as b:
            for (sx, sy, a), (rl, rr) in zip(probs, raggeds):
                b.add(sx, sy, a, rl, rr)
            b.upload()
            b.run()
            b.download()
            for i, ((sx, sy, a), (rl, rr)) in enumerate(zip(probs, raggeds)):
                want = ob.aligned_pairs(om, sx, sy, a, op, rl, rr)
                assert_pairs_match(b.result(i), want, threshold=op.threshold)


def _fuzz_problems(rng, n, expansion):
    probs, raggeds = [], []
    for _ in range(n):
        sx = _rand_seq(rng, rng.choice([0, 1, 5, 40, 150, 300]))
        sy = _evolve(rng, sx) if sx and rng.random() > 0.1 else _rand_seq(rng, rng.randrange(0, 80))
        anchors = []
        if rng.random() < 0.7 and sx and sy:
            step = rng.choice([1, 7, 30, 120])
            x = y = rng.randrange(0, 5)
            while x < len(sx) and y < len(sy):
                anchors.append((x, y, expansion))
                x += step + rng.randrange(0, 3)
                y += step + rng.randrange(0, 3)
        probs.append((sx, sy, anchors))
        raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
    return probs, raggeds


@pytest.mark.parametrize("seed", _fuzz_seeds([201, 202]))
def test_fuzz_batches_indel_and_expectation_emitters(seed):
    """The same kind of mixed batch through the other two emitters: three lists per problem (:691-733) against the oracle,
    and the batch's expectation counts (:735-746) against the oracle's sum over the problems (1e-5)."""
    rng = random.Random(seed)
    for mtype in (0, 2):
        tbd = rng.choice([1, 5, 40])
        pkw = dict(traceBackDiagonals=tbd, minDiagsBetweenTraceBack=tbd + rng.choice([2, 50, 960]),
                   diagonalExpansion=2 * rng.choice([2, 5, 10, 30]), splitMatrixBiggerThanThis=rng.choice([10, 10 ** 12]))
        probs, raggeds = _fuzz_problems(rng, 40, pkw["diagonalExpansion"])
        p, op, om = api.pairwiseAlignmentBandingParameters_construct(**pkw), ob.params(**pkw), ob.model(mtype)
        with api.Batch(_sm(mtype), p, emit=api.EMIT_INDEL) as b:
            for (sx, sy, a), (rl, rr) in zip(probs, raggeds):
                b.add(sx, sy, a, rl, rr)
            b.upload()
            b.run()
            b.download()
            for i, ((sx, sy, a), (rl, rr)) in enumerate(zip(probs, raggeds)):
                want = ob.aligned_pairs_with_indels(om, sx, sy, a, op, rl, rr)
                for which in range(3):
                    assert_pairs_match(b.result(i, which), want[which], threshold=op.threshold)
        acc, oacc = api.hmm_constructEmpty(0.0, mtype), ob.hmm(mtype, 0.0)
        with api.Batch(_sm(mtype), p, emit=api.EMIT_EXPECT) as b:
            for (sx, sy, a), (rl, rr) in zip(probs, raggeds):
                b.add(sx, sy, a, rl, rr)
            b.upload()
            b.run()
            b.download()
            b.expectations(acc)
        for (sx, sy, a), (rl, rr) in zip(probs, raggeds):
            ob.expectations(om, oacc, sx, sy, a, op, rl, rr)
        S = acc.stateNumber
        np.testing.assert_allclose(list(acc.transitions)[:S * S], list(oacc.T)[:S * S], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(list(acc.emissions)[:S * 16], list(oacc.E)[:S * 16], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(acc.likelihood, oacc.likelihood, rtol=1e-9)


def test_add_many_gives_the_same_results():
    """cpecan_batch_add_many (parallel, two passes) against cpecan_batch_add one problem at a time: identical lists."""
    rng = random.Random(301)
    pkw = dict(diagonalExpansion=10, splitMatrixBiggerThanThis=900)
    probs, raggeds = _fuzz_problems(rng, 200, 10)
    one, st1 = _run_batch(0, probs, raggeds, **pkw)
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
    with api.Batch(_sm(0), p) as b:
        assert b.add_many([(sx, sy, a, rl, rr) for (sx, sy, a), (rl, rr) in zip(probs, raggeds)]) == 0
        b.upload()
        b.run()
        b.download()
        st2 = b.stats()
        for i in range(len(probs)):
            assert np.array_equal(b.result(i), one[i])
    assert (st1.problems, st1.regions, st1.cells) == (st2.problems, st2.regions, st2.cells)


def test_concurrent_batches_from_host_threads():
    """Batches are independent objects: four host threads running their own small batches on the same device at the same
    time (recycled device blocks and shells behind one mutex, one error slot per thread) get what a single thread gets."""
    import threading
    rng = random.Random(401)
    pkw = dict(diagonalExpansion=10, splitMatrixBiggerThanThis=900)
    jobs = []
    for _ in range(24):
        probs, raggeds = _fuzz_problems(rng, rng.randrange(1, 12), 10)
        jobs.append((probs, raggeds))
    serial = [_run_batch(0, probs, raggeds, **pkw)[0] for probs, raggeds in jobs]
    results, errors = [None] * len(jobs), []

    def worker(tid):
        try:
            for j in range(tid, len(jobs), 4):
                for _ in range(3):  # the same job several times: blocks are recycled in between
                    results[j] = _run_batch(0, jobs[j][0], jobs[j][1], **pkw)[0]
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for got, want in zip(results, serial):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("mtype", [0, 3])
def test_random_wide_bands_stream_groups(mtype):
    """Diagonals of 65-250 cells with per-anchor expansions: two to four groups of 64 per diagonal, leftover cells
    sharing a group with the next diagonal in both sweep directions, direction switches at every anchor, short
    traceback schedules on top (the forward sweep treats the band as one stream of cells)."""
    rng = random.Random(77 + mtype)
    probs, raggeds = [], []
    for _ in range(16):
        sx = _rand_seq(rng, rng.randrange(150, 520))
        sy = _evolve(rng, sx) or "ACGT"
        anchors, x, y = [], -1, -1
        while True:
            x += rng.randrange(5, 90)
            y += rng.randrange(5, 90)
            if x >= len(sx) or y >= len(sy):
                break
            anchors.append((x, y, 2 * rng.randrange(20, 110)))
        probs.append((sx, sy, anchors))
        raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
    tbd = rng.randrange(3, 30)
    _check_batch(mtype, probs, raggeds, dynamicAnchorExpansion=1, traceBackDiagonals=tbd,
                 minDiagsBetweenTraceBack=tbd + rng.randrange(20, 200), splitMatrixBiggerThanThis=10 ** 12)
    _check_batch(mtype, probs[:6], raggeds[:6], diagonalExpansion=2 * rng.randrange(40, 100))


@pytest.mark.parametrize("mtype", [0, 2])
def test_ragged_ends_all_combinations(mtype):
    rng = random.Random(31 + mtype)
    core = _rand_seq(rng, 100)
    sy = _rand_seq(rng, 60) + core + _rand_seq(rng, 60)
    probs = [(core, sy, ())] * 4
    raggeds = [(False, False), (True, False), (False, True), (True, True)]
    _check_batch(mtype, probs, raggeds)


def test_multi_segment_tracebacks_default_schedule():
    # N > 2*minDiagsBetweenTraceBack so intermediate tracebacks fire with the default 1000/40 schedule
    problems = make_batch(3, 3, 2000, 100)
    worst, st = _check_batch(0, problems, diagonalExpansion=100)
    assert st.cells > 3 * 400000


def test_short_traceback_schedule_and_threshold_zero():
    sx, sy, a = make_pair(5, 0, 400, 10)
    _check_batch(0, [(sx, sy, a)], diagonalExpansion=10, minDiagsBetweenTraceBack=30, traceBackDiagonals=5)
    _check_batch(2, [(sx, sy, a)], diagonalExpansion=10, minDiagsBetweenTraceBack=12, traceBackDiagonals=1,
                 threshold=0.0)


def test_threshold_zero_five_segments_slice_is_not_multiplied(monkeypatch):
    """ADVICE r2 item 4 / VERDICT r3 item 8: with threshold <= 0 every cell is emitted.  A segment's part of the output
    slice is capped by the cells of ITS emitted diagonals (from the band walk), not by the whole region's cells: a 2 kb
    x 2 kb region of five segments used to ask for five times the triples it can ever fill.  Exact list equality with
    the oracle (every cell with x, y > 0, once), in both launch forms, and the device bytes stay near one region's."""
    sx, sy, a = make_pair(3, 1, 2000, 100)
    kw = dict(diagonalExpansion=100, threshold=0.0)
    om, op = ob.model(0), ob.params(**kw)
    want = ob.aligned_pairs(om, sx, sy, a, op, False, False)
    for form in ("0", "1"):
        monkeypatch.setenv("CPECAN_SPLIT", form)
        _, base = _run_batch(0, [(sx, sy, a)], diagonalExpansion=100)  # the default threshold: a slice of 6 (lX + lY) triples
        got, st = _run_batch(0, [(sx, sy, a)], **kw)
        assert st.regions == 1 and st.cells == base.cells and len(got[0]) == len(want)
        assert_pairs_match(got[0], want, threshold=0.0)
        assert np.array_equal(got[0][:, 1:], np.asarray(want)[:, 1:])  # the same cells in the same order
        assert len(want) > st.cells - 2 * 4002  # every band cell except those on the two zero edges
        # the triples (12 B) and their compact copy grow to one slice of `cells` triples each; five-fold slices (round 3)
        # were 4 * 24 * cells bytes more
        extra = st.deviceBytes - base.deviceBytes
        assert extra < 1.25 * 24 * st.cells, (form, extra, st.cells)


def test_run_form_anchors_and_closed_form_band_walk(monkeypatch):
    """VERDICT r3 item 4.  (a) cpecan_batch_add_many_runs takes the anchors as (x, y, length, expansion) runs of diagonal
    neighbours -- what cPecanRealign.c:525-529 + pairwiseAligner.c:979-1003 make of a cigar's match operations before they
    are expanded to one anchor per column -- and must give, bit for bit, what cpecan_batch_add_many gives on the expanded
    anchors.  (b) Planning walks such runs in closed form (cpecan_host.c, plan_region; the skip itself is the
    iterator's, cpk_band_skip_run in cpecan_band.inl): with CPECAN_FAST_WALK=0 every diagonal is walked one by one; cell counts, regions, device memory and every list must be
    the same -- also where traceback points fall inside runs (short schedules), at matrix edges (anchors from column 0), with
    split rectangles and with expansions 2 to 10.  And the oracle agrees on a sample."""
    from cpecan_amd import workload
    cases = []
    for E, seed in ((4, 11), (2, 12), (10, 13)):
        probs = workload.make_realign_batch(seed, 48, 60, 2500, expansion=E)
        cases.append((probs, dict(diagonalExpansion=E, splitMatrixBiggerThanThis=10), True))
        cases.append((probs[:24], dict(diagonalExpansion=E, splitMatrixBiggerThanThis=10, minDiagsBetweenTraceBack=120,
                                       traceBackDiagonals=17), True))
    # identical sequences: ONE run from corner to corner, traceback points deep inside it
    rng = random.Random(77)
    same = [(s, s, np.array([(i, i, 6) for i in range(len(s))], dtype=np.int64)) for s in
            (_rand_seq(rng, n) for n in (1, 2, 3, 40, 1500, 2600))]
    cases.append((same, dict(diagonalExpansion=6), False))
    cases.append((same, dict(diagonalExpansion=6, minDiagsBetweenTraceBack=200, traceBackDiagonals=40), False))
    for probs, kw, ragged in cases:
        p = api.pairwiseAlignmentBandingParameters_construct(**kw)
        problems = [(sx, sy, a, ragged, ragged) for sx, sy, a in probs]

        def run(runs):
            with api.Batch(_sm(0), p) as b:
                (b.add_many_runs if runs else b.add_many)(problems)
                b.upload()
                b.run()
                b.download()
                return [b.result(i).copy() for i in range(len(problems))], b.stats()

        monkeypatch.setenv("CPECAN_FAST_WALK", "0")
        slow, st0 = run(False)
        monkeypatch.delenv("CPECAN_FAST_WALK")
        fast, st1 = run(False)
        from_runs, st2 = run(True)
        for st in (st1, st2):
            assert (st.cells, st.regions, st.diagonals, st.pairs) == (st0.cells, st0.regions, st0.diagonals, st0.pairs)
        # (a batch that got runs keeps them as runs and expands them on the device: 16 bytes per run beside the anchors)
        assert st1.deviceBytes == st0.deviceBytes and st0.deviceBytes <= st2.deviceBytes <= st0.deviceBytes + 16 * st0.cells
        # ... unless told to expand them on the host as rounds 1-3 did (CPECAN_KEEP_RUNS=0): the same lists
        monkeypatch.setenv("CPECAN_KEEP_RUNS", "0")
        expanded, st3 = run(True)
        monkeypatch.delenv("CPECAN_KEEP_RUNS")
        assert st3.deviceBytes == st0.deviceBytes
        for a0, a3 in zip(slow, expanded):
            assert np.array_equal(a0, a3)
        # one batch, both forms: the form of the first problems decides what the batch keeps -- runs first: the anchors that
        # come one by one behind them become runs of one; anchors first: the runs behind them are expanded on the host
        half = len(problems) // 2
        for runs_first in (True, False):
            with api.Batch(_sm(0), p) as b:
                if runs_first:
                    b.add_many_runs(problems[:half])
                    b.add_many(problems[half:])
                else:
                    b.add_many(problems[:half])
                    b.add_many_runs(problems[half:])
                b.upload()
                b.run()
                b.download()
                for i in range(len(problems)):
                    assert np.array_equal(slow[i], b.result(i)), ("mixed forms", runs_first, i)
        for i, (a0, a1, a2) in enumerate(zip(slow, fast, from_runs)):
            assert np.array_equal(a0, a1), ("closed-form walk", i)
            assert np.array_equal(a0, a2), ("run form", i)
        om, op = ob.model(0), ob.params(**kw)
        for i in range(0, len(problems), max(1, len(problems) // 6)):
            sx, sy, a, rl, rr = problems[i]
            assert_pairs_match(from_runs[i], ob.aligned_pairs(om, sx, sy, a, op, rl, rr), threshold=op.threshold)
    # bad runs are refused like bad anchors
    with api.Batch(_sm(0), api.pairwiseAlignmentBandingParameters_construct()) as b:
        for bad in ([(0, 0, 0, 4)], [(0, 0, 5, 4)], [(2, 2, 1, 4), (2, 3, 1, 4)], [(-1, 0, 1, 4)]):
            arr = (api.ProblemRuns * 1)()
            runs = np.array(bad, dtype=np.int64)
            arr[0].sX, arr[0].lX, arr[0].sY, arr[0].lY = b"ACGT", 4, b"ACGT", 4
            arr[0].runs, arr[0].nRuns = runs.ctypes.data_as(api.C.POINTER(api.C.c_int64)), len(bad)
            with pytest.raises(api.CpecanError):
                b.add_prepared(arr, 1)


def test_split_by_large_gaps_regions():
    # cPecanRealign-style: tiny split threshold, small expansion, ragged ends (cPecanRealign.c:355-357,537)
    rng = random.Random(41)
    sx = _rand_seq(rng, 500)
    sy = _evolve(rng, sx)
    n = min(len(sx), len(sy))
    anchors = [(i, i, 4) for i in range(5, n - 5, 29)]
    _check_batch(0, [(sx, sy, anchors)], [(True, True)], diagonalExpansion=4, splitMatrixBiggerThanThis=10)
    _check_batch(0, [(sx, sy, anchors)], [(False, False)], diagonalExpansion=4, splitMatrixBiggerThanThis=400)


def test_hmm_loaded_models():
    rng = random.Random(51)
    for mtype in (0, 1, 2, 3):
        ph, oh = api.hmm_constructEmpty(0.0, mtype), ob.hmm(mtype, 0.0)
        S = ph.stateNumber
        for i in range(S * S):
            ph.transitions[i] = oh.T[i] = 0.05 + rng.random()
        for i in range(S * 16):
            ph.emissions[i] = oh.E[i] = 0.05 + rng.random()
        api.hmm_normalise(ph)
        ob.lib().orc_hmm_normalise(oh)
        sx = _rand_seq(rng, 150)
        sy = _evolve(rng, sx)
        p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=30)
        got = api.getAlignedPairsUsingAnchors(api.hmm_getStateMachine(ph), sx, sy, (), p)
        want = ob.aligned_pairs(ob.model_from_hmm(oh), sx, sy, (), ob.params(diagonalExpansion=30))
        assert_pairs_match(got, want, threshold=p.threshold)


def test_config_A_sample_three_state_band50():
    # BASELINE configs[1] shape (1 kb x 1 kb, stateMachine3, band 50) on a 24-pair sample
    problems = make_batch(2, 24, 1000, 50)
    worst, st = _check_batch(2, problems, diagonalExpansion=50)
    assert st.regions == 24


def test_config_B_sample_five_state_band100():
    # BASELINE configs[2] shape (2 kb x 2 kb, stateMachine5, band 100) on a 12-pair sample
    problems = make_batch(3, 12, 2000, 100, first=100)
    _check_batch(0, problems, diagonalExpansion=100)


def test_wide_band_uses_global_rolling_buffers():
    # 1500 x 1500 without anchors: diagonals up to 1501 cells -> rolling buffers exceed the LDS budget
    sx, sy, _ = make_pair(7, 0, 1500, 0)
    _check_batch(0, [(sx, sy, ())], diagonalExpansion=20)


@pytest.mark.parametrize("mtype,emit", [(0, "match"), (2, "match"), (0, "expect")])
def test_mixed_widths_run_in_size_classes(mtype, emit):
    """One batch with regions of every wide class -- banded at 41-81 cells, unanchored 150 x 150 (151 cells), 300 x 300
    (301), 500 x 500 (501) and 900 x 900 (901 cells: rolling buffers in global memory for one wave; the match emitter
    runs the last two on the team kernel) -- runs as one launch per class, each with LDS and scratch for its own largest
    region, and gives what each problem gives alone."""
    probs = [make_pair(31, i, 400, 40) for i in range(40)]                       # <= 128 cells
    probs += [make_pair(32, i, 150, 0)[:2] + ((),) for i in range(6)]            # <= 256
    probs += [make_pair(33, i, 300, 0)[:2] + ((),) for i in range(4)]            # fits the LDS
    probs += [make_pair(36, i, 500, 0)[:2] + ((),) for i in range(2)]            # 501 cells: a team of four waves (match emitter)
    probs += [make_pair(34, 0, 900, 0)[:2] + ((),)]                              # 901: does not fit one wave's LDS; a team of eight
    probs += [make_pair(35, i, 200, 40) for i in range(80)]                      # more of the first class, behind the wide ones
    pkw = dict(diagonalExpansion=40)
    if emit == "match":
        worst, st = _check_batch(mtype, probs, **pkw)
        assert st.regions == len(probs)
        # the batch composition does not change a result
        alone, _ = _run_batch(mtype, probs[46:53], **pkw)
        together, _ = _run_batch(mtype, probs, **pkw)
        for t1, t2 in zip(alone, together[46:53]):
            assert np.array_equal(t1, t2)
    else:
        p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
        acc = api.hmm_constructEmpty(0.0, mtype)
        with api.Batch(_sm(mtype), p, emit=api.EMIT_EXPECT) as b:
            for sx, sy, a in probs:
                b.add(sx, sy, a, False, False)
            b.upload()
            b.run()
            b.download()
            b.expectations(acc)
        oacc = ob.hmm(mtype, 0.0)
        om, op = ob.model(mtype), ob.params(**pkw)
        for sx, sy, a in probs:
            ob.expectations(om, oacc, sx, sy, a, op, False, False)
        S = acc.stateNumber
        np.testing.assert_allclose(list(acc.transitions)[:S * S], list(oacc.T)[:S * S], rtol=1e-5)
        np.testing.assert_allclose(list(acc.emissions)[:S * 16], list(oacc.E)[:S * 16], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(acc.likelihood, oacc.likelihood, rtol=1e-9)


def test_output_overflow_triggers_exact_rerun():
    sx, sy, a = make_pair(8, 0, 300, 40)
    got, st = _run_batch(0, [(sx, sy, a)], diagonalExpansion=40, threshold=1e-9)
    want = ob.aligned_pairs(ob.model(0), sx, sy, a, ob.params(diagonalExpansion=40, threshold=1e-9))
    assert_pairs_match(got[0], want, threshold=1e-9)


def test_memory_budget_caps_resident_waves(monkeypatch):
    """Every resident wave owns scratch sized for the batch's largest region; when that does not fit in device memory the
    batch runs with fewer waves (the other regions queue) and gives the same lists.  CPECAN_MEM_BUDGET_MB stands in for
    a nearly full device; a budget below one wave's scratch is an error, not a crash."""
    problems = make_batch(21, 300, 400, 40)
    free, st_free = _run_batch(0, problems, diagonalExpansion=40)
    monkeypatch.setenv("CPECAN_MEM_BUDGET_MB", "120")
    capped, st_capped = _run_batch(0, problems, diagonalExpansion=40)
    assert 1 <= st_capped.wavesPerLaunch < st_free.wavesPerLaunch
    for t1, t2 in zip(free, capped):
        assert np.array_equal(t1, t2)
    monkeypatch.setenv("CPECAN_MEM_BUDGET_MB", "1")
    with pytest.raises(api.CpecanError) as e:
        _run_batch(0, problems, diagonalExpansion=40)
    assert "out of device memory" in str(e.value)


def test_full_size_properties_config_B_slice():
    """Size-independent properties at BASELINE's full per-pair size: scores in (0, 1e7], coordinates unique and
    in range, per-row posterior mass <= 1 (+ logAdd slack), and results independent of batch composition."""
    problems = make_batch(3, 64, 2000, 100, first=500)
    got, st = _run_batch(0, problems, diagonalExpansion=100)
    for (sx, sy, a), tri in zip(problems, got):
        assert len(tri) > 0.9 * min(len(sx), len(sy))
        assert tri[:, 0].min() > 0 and tri[:, 0].max() <= api.PAIR_ALIGNMENT_PROB_1
        assert tri[:, 1].min() >= 0 and tri[:, 1].max() < len(sx)
        assert tri[:, 2].min() >= 0 and tri[:, 2].max() < len(sy)
        assert len({(int(x), int(y)) for _, x, y in tri}) == len(tri)
        rowmass = np.bincount(tri[:, 1], weights=tri[:, 0], minlength=len(sx))
        assert rowmass.max() <= 1.01 * api.PAIR_ALIGNMENT_PROB_1
    again, _ = _run_batch(0, problems[10:20], diagonalExpansion=100)
    for t1, t2 in zip(got[10:20], again):
        assert np.array_equal(t1, t2)


# ---- indel emitter (diagonalCalculationPosteriorProbs, pairwiseAligner.c:691-733) ----

def _check_indels(mtype, sx, sy, anchors, rl=False, rr=False, **pkw):
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
    got = api.getAlignedPairsWithIndelsUsingAnchors(_sm(mtype), sx, sy, anchors, p, rl, rr)
    want = ob.aligned_pairs_with_indels(ob.model(mtype), sx, sy, anchors, ob.params(**pkw), rl, rr)
    for g, w in zip(got, want):
        assert_pairs_match(g, w, threshold=p.threshold)
    return got


@pytest.mark.parametrize("mtype", [0, 2])
def test_indel_emitter_matches_oracle(mtype):
    # tests/pairwiseAlignerTest.c:867-942 uses stateMachine3; both models here
    rng = random.Random(61 + mtype)
    for _ in range(6):
        sx = _rand_seq(rng, rng.randrange(1, 120))
        sy = _evolve(rng, sx)
        match, gapx, gapy = _check_indels(mtype, sx, sy, (), bool(rng.random() > 0.5), bool(rng.random() > 0.5))
        if len(gapx):
            assert gapx[:, 1].min() >= 0 and gapx[:, 2].min() >= -1
        if len(gapy):
            assert gapy[:, 1].min() >= -1 and gapy[:, 2].min() >= 0
    sx, sy, a = make_pair(9, 0, 1200, 30)
    _check_indels(mtype, sx, sy, a, diagonalExpansion=30)  # multi-segment


@pytest.mark.parametrize("mtype", [0, 2])
def test_indel_emitter_on_the_team_kernel(mtype, monkeypatch):
    """Round 4: the three lists of the indel emitter (pairwiseAligner.c:691-733) from the team of waves that wide bands go
    to -- an unanchored 500 x 500 pair (501 cells: four waves) and, five-state, 900 x 900 (eight waves) by the library's own
    choice, and a multi-segment band of ~157 cells forced onto the team (CPECAN_TEAM=100): each equal to the oracle's lists
    and, list for list, to what one wave per region gives (CPECAN_TEAM=0)."""
    cases = [(make_pair(36, 0, 500, 0)[:2] + ((),), dict(diagonalExpansion=40), None)]
    if mtype == 0:
        cases.append((make_pair(34, 0, 900, 0)[:2] + ((),), dict(diagonalExpansion=40), None))
    cases.append((make_pair(3, 5, 1500, 100), dict(diagonalExpansion=100), "100"))
    for (sx, sy, a), pkw, team in cases:
        if team:
            monkeypatch.setenv("CPECAN_TEAM", team)
        else:
            monkeypatch.delenv("CPECAN_TEAM", raising=False)
        teamed = _check_indels(mtype, sx, sy, a, True, False, **pkw)
        monkeypatch.setenv("CPECAN_TEAM", "0")
        solo = api.getAlignedPairsWithIndelsUsingAnchors(_sm(mtype), sx, sy, a, api.pairwiseAlignmentBandingParameters_construct(**pkw),
                                                         True, False)
        for t, o in zip(teamed, solo):
            assert np.array_equal(t, o)
    monkeypatch.delenv("CPECAN_TEAM", raising=False)


@pytest.mark.parametrize("mtype", [0, 3])
def test_expectation_emitter_on_the_team_kernel(mtype, monkeypatch):
    """Round 4: expectations from the team of waves wide bands go to -- the traceback parks B of the emitted cells, wave 0
    folds the totals, the waves share the second pass.  Unanchored 500 x 500 (a team of four) and 900 x 900 pairs (eight; the
    five-state model by the library's own choice) and a multi-segment band forced onto the team (CPECAN_TEAM=100), several
    regions per launch: counts and likelihood within 1e-5 of the oracle's and within 1e-9 of one wave per region's
    (CPECAN_TEAM=0; the order of the sums differs)."""
    cases = [([make_pair(36, i, 500, 0)[:2] + ((),) for i in range(3)] + [make_pair(34, 0, 900, 0)[:2] + ((),)], dict(diagonalExpansion=40), None),
             ([make_pair(3, 5 + i, 1500, 100) for i in range(3)], dict(diagonalExpansion=100), "100"),
             # a class narrow enough for the events inside the traceback (<= 128 cells), forced onto the team: the team's
             # second pass needs B of the emitted cells, not the window records (tools/soak_emitters.py, seed 5 round 0)
             ([make_pair(8, i, 700, 60, anchor_every=150) for i in range(5)],
              dict(diagonalExpansion=60, traceBackDiagonals=12, minDiagsBetweenTraceBack=300), "100")]
    for probs, pkw, team in cases:
        p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
        accs = []
        for env in (team, "0"):
            if env is None:
                monkeypatch.delenv("CPECAN_TEAM", raising=False)
            else:
                monkeypatch.setenv("CPECAN_TEAM", env)
            acc = api.hmm_constructEmpty(0.0, mtype)
            with api.Batch(_sm(mtype), p, emit=api.EMIT_EXPECT) as b:
                for sx, sy, a in probs:
                    b.add(sx, sy, a, True, False)
                b.upload()
                b.run()
                b.download()
                b.expectations(acc)
            accs.append(acc)
        oacc = ob.hmm(mtype, 0.0)
        om, op = ob.model(mtype), ob.params(**pkw)
        for sx, sy, a in probs:
            ob.expectations(om, oacc, sx, sy, a, op, True, False)
        S = accs[0].stateNumber
        for acc, rtol in ((accs[0], 1e-5), (accs[1], 1e-5)):
            np.testing.assert_allclose(list(acc.transitions)[:S * S], list(oacc.T)[:S * S], rtol=rtol)
            np.testing.assert_allclose(list(acc.emissions)[:S * 16], list(oacc.E)[:S * 16], rtol=rtol, atol=1e-12)
            np.testing.assert_allclose(acc.likelihood, oacc.likelihood, rtol=1e-9)
        np.testing.assert_allclose(list(accs[0].transitions)[:S * S], list(accs[1].transitions)[:S * S], rtol=1e-9)
        np.testing.assert_allclose(list(accs[0].emissions)[:S * 16], list(accs[1].emissions)[:S * 16], rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(accs[0].likelihood, accs[1].likelihood, rtol=1e-12)
    monkeypatch.delenv("CPECAN_TEAM", raising=False)


def test_indel_emitter_match_list_equals_match_emitter():
    sx, sy, a = make_pair(9, 1, 500, 20)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=20)
    m1 = api.getAlignedPairsUsingAnchors(_sm(0), sx, sy, a, p)
    m2, _, _ = api.getAlignedPairsWithIndelsUsingAnchors(_sm(0), sx, sy, a, p)
    assert np.array_equal(m1, m2)


# ---- forward probability (computeForwardProbability, pairwiseAligner.c:936) ----

def test_forward_probability_known_answers():
    # SURVEY 8c known answers from the reference
    p = api.pairwiseAlignmentBandingParameters_construct()
    assert abs(api.computeForwardProbability("AGCG", "AGTTCG", (), p, api.stateMachine5_construct()) + 17.519321161239) < 1e-11
    assert abs(api.computeForwardProbability("AGCG", "AGTTCG", (), p, api.stateMachine3_construct()) + 17.381039440328) < 1e-11
    assert abs(api.computeForwardProbability("AGCG", "AGTTCG", (), p, api.stateMachine3_construct(), True, True)
               + 20.651524037167) < 1e-11
    assert api.computeForwardProbability("", "", (), p, api.stateMachine3_construct()) == 0.0


def test_forward_probability_matches_oracle_and_reference_properties():
    # tests/pairwiseAlignerTest.c:1157-1188
    rng = random.Random(71)
    sm, om = api.stateMachine3_construct(), ob.model(2)
    p, op = api.pairwiseAlignmentBandingParameters_construct(), ob.params()
    with api.Batch(sm, p, emit=api.EMIT_FORWARD) as b:
        cases = []
        for _ in range(40):
            sx = _rand_seq(rng, rng.randrange(10, 100))
            sy = _evolve(rng, sx)
            rl, rr = rng.random() > 0.5, rng.random() > 0.5
            cases.append((sx, sy, rl, rr))
            b.add(sx, sy, (), rl, rr)
            b.add(sx, sx, (), rl, rr)
        b.upload()
        b.run()
        b.download()
        for i, (sx, sy, rl, rr) in enumerate(cases):
            lp, lpi = b.forward_prob(2 * i), b.forward_prob(2 * i + 1)
            assert_log_close(lp, ob.forward_prob(om, sx, sy, (), op, rl, rr))  # pure logAdd arithmetic
            assert_log_close(lpi, ob.forward_prob(om, sx, sx, (), op, rl, rr))
            assert float("-inf") < lp <= 0.0 and lp <= lpi
    sx, sy, a = make_pair(10, 0, 1500, 40)
    p5 = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=40, dynamicAnchorExpansion=1)
    got = api.computeForwardProbability(sx, sy, a, p5, api.stateMachine5_construct())
    assert_log_close(got, ob.forward_prob(ob.model(0), sx, sy, a, ob.params(diagonalExpansion=40, dynamicAnchorExpansion=1)))


# ---- expectation emitter (diagonalCalculationExpectations, pairwiseAligner.c:735-746) ----

def _assert_hmm_close(got, want, S, rel=1e-5):
    for i in range(S * S):
        assert abs(got.transitions[i] - want.T[i]) <= rel * abs(want.T[i]) + 1e-12, ("T", i, got.transitions[i], want.T[i])
    for i in range(S * 16):
        assert abs(got.emissions[i] - want.E[i]) <= rel * abs(want.E[i]) + 1e-12, ("E", i, got.emissions[i], want.E[i])
    assert abs(got.likelihood - want.likelihood) <= rel * abs(want.likelihood) + 1e-9


def test_expectations_known_answers():
    # 5-state, pseudo count 0, AGCG vs AGTTCG
    h = api.hmm_constructEmpty(0.0, api.fiveState)
    api.getExpectationsUsingAnchors(api.stateMachine5_construct(), h, "AGCG", "AGTTCG", (),
                                    api.pairwiseAlignmentBandingParameters_construct())
    # (the events are exp2f(fp32 argument): ~1e-7 relative each, against north_star's 1e-5)
    assert abs(h.likelihood + 175.193211612) < 1e-8
    assert abs(h.transitions[0] - 3.010391804) < 1e-7
    assert abs(h.transitions[1] - 0.000751913) < 1e-8
    assert abs(h.emissions[0] - 0.994467322) < 1e-7


@pytest.mark.parametrize("second_pass", [False, True])
@pytest.mark.parametrize("mtype", [0, 1, 2, 3])
def test_expectations_match_oracle(mtype, second_pass, monkeypatch):
    # bands of up to 128 cells form the events inside the traceback (Sweep::tracebackExpect); CPECAN_EXP_INSWEEP=0 sends
    # them through the second pass that wider bands take (Sweep::expectations)
    # (2: inside the traceback whatever the LDS costs -- the library's own choice depends on the band width and the model)
    monkeypatch.setenv("CPECAN_EXP_INSWEEP", "0" if second_pass else "2")
    rng = random.Random(81 + mtype)
    ph, oh = api.hmm_constructEmpty(0.0, mtype), ob.hmm(mtype, 0.0)
    S = ph.stateNumber
    for i in range(S * S):
        ph.transitions[i] = oh.T[i] = 0.05 + rng.random()
    for i in range(S * 16):
        ph.emissions[i] = oh.E[i] = 0.05 + rng.random()
    api.hmm_normalise(ph)
    ob.lib().orc_hmm_normalise(oh)
    sm, om = api.hmm_getStateMachine(ph), ob.model_from_hmm(oh)
    problems = [(_rand_seq(rng, rng.randrange(10, 100)),) for _ in range(6)]
    problems = [(sx, _evolve(rng, sx), ()) for (sx,) in problems]
    sx, sy, a = make_pair(11, mtype, 1300, 20)  # several traceback segments: exercises the freed-F[d-2] quirk
    problems.append((sx, sy, a))
    kw = dict(diagonalExpansion=20)
    acc_g, acc_o = api.hmm_constructEmpty(1e-12, mtype), ob.hmm(mtype, 1e-12)
    with api.Batch(sm, api.pairwiseAlignmentBandingParameters_construct(**kw), emit=api.EMIT_EXPECT) as b:
        for sx, sy, a in problems:
            b.add(sx, sy, a, True, False)
        b.upload()
        b.run()
        b.download()
        b.expectations(acc_g)
    for sx, sy, a in problems:
        ob.expectations(om, acc_o, sx, sy, a, ob.params(**kw), True, False)
    _assert_hmm_close(acc_g, acc_o, S)


def test_expectations_wide_band_takes_second_pass():
    # an unanchored 260 x 240 pair: diagonals of up to 241 cells, beyond what the in-traceback events cover
    rng = random.Random(7)
    sx = _rand_seq(rng, 260)
    sy = _evolve(rng, sx)[:240]
    mtype = api.fiveState
    sm, om = api.stateMachine5_construct(), ob.model(mtype)
    acc_g, acc_o = api.hmm_constructEmpty(1e-12, mtype), ob.hmm(mtype, 1e-12)
    api.getExpectationsUsingAnchors(sm, acc_g, sx, sy, (), api.pairwiseAlignmentBandingParameters_construct())
    ob.expectations(om, acc_o, sx, sy, (), ob.params(), False, False)
    _assert_hmm_close(acc_g, acc_o, acc_g.stateNumber)


def test_em_iterations_likelihood_monotone_on_gpu():
    # tests/pairwiseAlignerTest.c:1091-1143 (test_em), 3-state, on the HIP path
    rng = random.Random(91)
    sx = _rand_seq(rng, 80)
    sy = _evolve(rng, sx)
    h = api.hmm_constructEmpty(0.0, api.threeState)
    for i in range(9):
        h.transitions[i] = rng.random()
    for i in range(48):
        h.emissions[i] = rng.random()
    api.hmm_normalise(h)
    sm = api.hmm_getStateMachine(h)
    p = api.pairwiseAlignmentBandingParameters_construct()
    prev = float("-inf")
    for _ in range(6):
        acc = api.hmm_constructEmpty(1e-12, api.threeState)
        api.getExpectationsUsingAnchors(sm, acc, sx, sy, (), p)
        api.hmm_normalise(acc)
        assert prev <= acc.likelihood * 0.95
        prev = acc.likelihood
        sm = api.hmm_getStateMachine(acc)


def test_expectation_step_helper_single_rank():
    """cpecan_amd.dist.expectation_step on one GPU (world size 1: the all-reduce is the identity)."""
    from cpecan_amd import dist as cdist
    problems = make_batch(5, 6, 150, 10)
    sm = api.stateMachine5_construct()
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=10)
    acc = cdist.expectation_step(sm, [(sx, sy, a, True, True) for sx, sy, a in problems], p, pseudo=1e-12)
    oacc = ob.hmm(ob.FIVE_STATE, 1e-12)
    for sx, sy, a in problems:
        ob.expectations(ob.model(0), oacc, sx, sy, a, ob.params(diagonalExpansion=10), True, True)
    _assert_hmm_close(acc, oacc, 5)


# ---- BASELINE configs 4 and 5 on samples ----

def test_config4_realign_sample_mixed_lengths_split_regions():
    """configs[3]: cPecanRealign mode -- mixed lengths, anchors on every exact-match column, diagonalExpansion 4,
    splitMatrixBiggerThanThis 10, ragged ends (cPecanRealign.c:355-357, 537).  40-pair sample vs the oracle."""
    from cpecan_amd.workload import make_realign_batch
    problems = make_realign_batch(4, 40, 100, 3000, 4)
    kw = dict(diagonalExpansion=4, splitMatrixBiggerThanThis=10)
    worst, st = _check_batch(0, problems, [(True, True)] * len(problems), **kw)
    assert st.regions >= len(problems)  # anchor gaps whose matrix exceeds 10 cells open extra regions


def test_config5_expectation_sample_band10():
    """configs[4]: EM expectation step, 1 kb pairs, diagonalExpansion 10; 48-pair sample vs the oracle."""
    problems = make_batch(5, 48, 1000, 10)
    kw = dict(diagonalExpansion=10)
    acc = api.hmm_constructEmpty(1e-12, api.fiveState)
    with api.Batch(api.stateMachine5_construct(), api.pairwiseAlignmentBandingParameters_construct(**kw),
                   emit=api.EMIT_EXPECT) as b:
        for sx, sy, a in problems:
            b.add(sx, sy, a, True, True)
        b.upload()
        b.run()
        b.download()
        b.expectations(acc)
    oacc = ob.hmm(ob.FIVE_STATE, 1e-12)
    for sx, sy, a in problems:
        ob.expectations(ob.model(0), oacc, sx, sy, a, ob.params(**kw), True, True)
    _assert_hmm_close(acc, oacc, 5)


@pytest.mark.parametrize("name", ["A", "B"])
def test_configs_A_and_B_at_full_size(name):
    """configs[1] and configs[2] with every pair of the BASELINE batch in ONE launch, as bench.py runs them (config A:
    a split class, tracebacks as queue items of their own): a sample spread over the batch against the oracle, and a
    slice run again in a batch of its own -- identical lists."""
    from cpecan_amd import workload
    cfg = workload.CONFIGS[name]
    n, mtype = cfg["n_pairs"], (0 if cfg["model"] == "fiveState" else 2)
    problems = workload.config_problems(name, range(n))
    kw = dict(diagonalExpansion=cfg["expansion"])
    p = api.pairwiseAlignmentBandingParameters_construct(**kw)
    with api.Batch(_sm(mtype), p) as b:
        b.add_many(problems)
        b.upload()
        b.run()
        b.download()
        st = b.stats()
        assert st.problems == n
        om, op = ob.model(mtype), ob.params(**kw)
        for i in sorted(set(range(0, n, n // 12)) | {n - 1}):
            sx, sy, a, rl, rr = problems[i]
            assert_pairs_match(b.result(i), ob.aligned_pairs(om, sx, sy, a, op, rl, rr), threshold=op.threshold)
        keep = [b.result(i).copy() for i in range(n // 2, n // 2 + 40)]
        assert sum(len(b.result(i)) for i in range(n)) == st.pairs
    again, _ = _run_batch(mtype, [pr[:3] for pr in problems[n // 2:n // 2 + 40]], **kw)
    for t1, t2 in zip(keep, again):
        assert np.array_equal(t1, t2)


def test_config4_at_full_size():
    """configs[3] at BASELINE's size -- all 50 000 pairs in ONE batch, as bench.py runs it: a sample spread over the batch
    (the longest pair included) against the oracle, every list's size-independent properties, and a slice of the batch
    run again in a batch of its own (other size classes, other wave slots): identical lists."""
    from cpecan_amd import workload
    cfg = workload.CONFIGS["4"]
    n = cfg["n_pairs"]
    problems = workload.config_problems("4", range(n))
    kw = dict(diagonalExpansion=cfg["expansion"], splitMatrixBiggerThanThis=cfg["split"])
    p = api.pairwiseAlignmentBandingParameters_construct(**kw)
    with api.Batch(_sm(0), p) as b:
        b.add_many(problems)
        b.upload()
        b.run()
        b.download()
        st = b.stats()
        assert st.problems == n and st.regions >= n
        longest = max(range(n), key=lambda i: len(problems[i][0]))
        sample = sorted(set(range(0, n, n // 24)) | {longest, n - 1})
        om, op = ob.model(0), ob.params(**kw)
        for i in sample:
            sx, sy, a, rl, rr = problems[i]
            assert_pairs_match(b.result(i), ob.aligned_pairs(om, sx, sy, a, op, rl, rr), threshold=op.threshold)
        total = 0
        for i in range(n):
            tri = b.result(i)
            total += len(tri)
            if len(tri) == 0:
                continue
            sx, sy = problems[i][0], problems[i][1]
            assert tri[:, 0].min() > 0 and tri[:, 0].max() <= api.PAIR_ALIGNMENT_PROB_1
            assert tri[:, 1].min() >= 0 and tri[:, 1].max() < len(sx) and tri[:, 2].min() >= 0 and tri[:, 2].max() < len(sy)
            assert len(np.unique(tri[:, 1].astype(np.int64) * (len(sy) + 1) + tri[:, 2])) == len(tri)
        assert total == st.pairs
        keep = [b.result(i).copy() for i in range(3000, 3400)]
    again, _ = _run_batch(0, [pr[:3] for pr in problems[3000:3400]], [(True, True)] * 400, **kw)
    for t1, t2 in zip(keep, again):
        assert np.array_equal(t1, t2)


def test_config5_at_full_size_counts_add_up():
    """configs[4] at BASELINE's size: the expectation counts of all 100 000 pairs in one batch equal the sum of the counts
    of four quarters run as batches of their own (the counts are sums over cells: additive whatever the batching), and a
    sample of the pairs agrees with the oracle (test_config5_expectation_sample_band10 does the oracle side)."""
    from cpecan_amd import workload
    cfg = workload.CONFIGS["5"]
    n = cfg["n_pairs"]
    problems = workload.config_problems("5", range(n))
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=cfg["expansion"])

    def counts(probs):
        acc = api.hmm_constructEmpty(0.0, api.fiveState)
        with api.Batch(api.stateMachine5_construct(), p, emit=api.EMIT_EXPECT) as b:
            b.add_many(probs)
            b.upload()
            b.run()
            b.download()
            b.expectations(acc)
        return np.array(list(acc.transitions[:25]) + list(acc.emissions[:80]) + [acc.likelihood])

    whole = counts(problems)
    parts = sum(counts(problems[k * n // 4:(k + 1) * n // 4]) for k in range(4))
    assert np.all(np.isfinite(whole)) and whole[:25].sum() > n * 1000  # about one transition per cell of the path
    np.testing.assert_allclose(whole, parts, rtol=1e-9, atol=1e-6)


# ---- narrow bands: the packed kernel (several regions per wave) ----
@pytest.fixture
def force_packed(monkeypatch):
    monkeypatch.setenv("CPECAN_PACKED", "2")  # also for batches of fewer than 64 narrow regions


@pytest.mark.parametrize("mtype", [0, 2])
def test_packed_kernel_realign_sample(force_packed, mtype):
    """BASELINE config 4 in miniature through the packed kernel: expansion 4, anchors on every matching column, ragged
    ends, split at 10 (cPecanRealign.c:355-357), lengths 100-3000 (several traceback segments for the long ones)."""
    from cpecan_amd.workload import make_realign_batch
    problems = make_realign_batch(4, 70, 100, 3000, 4)
    worst, st = _check_batch(mtype, problems, [(True, True)] * len(problems), diagonalExpansion=4,
                             splitMatrixBiggerThanThis=10)
    assert st.regions >= len(problems)


@pytest.mark.parametrize("mtype", [0, 2])
def test_packed_kernel_per_anchor_expansions(force_packed, mtype):
    """dynamicAnchorExpansion (band_constructDynamic, pairwiseAligner.c:184-234) through the packed kernel's DYN variant:
    every anchor brings an expansion of its own (0-24: group widths 8 to 32), so the band's edges move back where a larger
    one follows a smaller one; dense and sparse anchors (a sparse stretch makes the band wander further than a symbol window
    holds: those cells read global memory), short traceback schedules, match and expectation emitters."""
    rng = random.Random(57 + mtype)
    probs, raggeds = [], []
    for k in range(40):
        sx = _rand_seq(rng, rng.randrange(1, 700))
        sy = _evolve(rng, sx) or "A"
        anchors, x, y = [], -1, -1
        while True:
            step = rng.randrange(1, 5) if k % 3 else rng.randrange(1, 4)
            x += step
            y += step if rng.random() < 0.8 else rng.randrange(1, 5)
            if x >= len(sx) or y >= len(sy):
                break
            anchors.append((x, y, 2 * rng.randrange(0, 13)))
        probs.append((sx, sy, anchors))
        raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
    tbd = rng.randrange(2, 12)
    worst, st = _check_batch(mtype, probs, raggeds, dynamicAnchorExpansion=1, traceBackDiagonals=tbd,
                             minDiagsBetweenTraceBack=tbd + rng.randrange(20, 150), splitMatrixBiggerThanThis=10 ** 12)
    # and the expectation emitter on the same bands, against the oracle
    kw = dict(dynamicAnchorExpansion=1)
    acc_g, acc_o = api.hmm_constructEmpty(1e-12, mtype), ob.hmm(mtype, 1e-12)
    with api.Batch(_sm(mtype), api.pairwiseAlignmentBandingParameters_construct(**kw), emit=api.EMIT_EXPECT) as b:
        for (sx, sy, a), (rl, rr) in zip(probs, raggeds):
            b.add(sx, sy, a, rl, rr)
        b.upload()
        b.run()
        b.download()
        b.expectations(acc_g)
    om = ob.model(mtype)
    for (sx, sy, a), (rl, rr) in zip(probs, raggeds):
        ob.expectations(om, acc_o, sx, sy, a, ob.params(**kw), rl, rr)
    _assert_hmm_close(acc_g, acc_o, acc_g.stateNumber)


def test_packed_kernel_random_narrow_bands(force_packed):
    """Group widths 8, 16 and 32; random anchors and traceback schedules; mixed with wide regions in one batch."""
    rng = random.Random(91)
    for exp, hi in ((2, 300), (8, 400), (20, 500)):
        probs, raggeds = [], []
        for _ in range(24):
            sx = _rand_seq(rng, rng.randrange(1, hi))
            sy = _evolve(rng, sx) or "A"
            anchors, x, y = [], -1, -1
            while True:
                x += rng.randrange(1, 6)
                y += rng.randrange(1, 6)
                if x >= len(sx) or y >= len(sy):
                    break
                anchors.append((x, y, exp))
            probs.append((sx, sy, anchors))
            raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
        # two wide regions ride along: they must take the one-wave-per-region kernel
        probs += [(_rand_seq(rng, 120), _rand_seq(rng, 130), [])] * 2
        raggeds += [(False, False)] * 2
        tbd = rng.randrange(2, 12)
        _check_batch(0, probs, raggeds, diagonalExpansion=exp, traceBackDiagonals=tbd,
                     minDiagsBetweenTraceBack=tbd + rng.randrange(3, 60), splitMatrixBiggerThanThis=10 ** 12)


def test_packed_and_sweep_kernels_agree_bit_for_bit(monkeypatch):
    """The packed kernel runs the sweep kernel's own cell functions: the same batch through either must give identical
    triples (not just within tolerance), for all three group widths and both model families."""
    rng = random.Random(123)
    for mtype, exp in ((0, 2), (2, 6), (1, 14), (3, 26)):
        probs, raggeds = [], []
        for _ in range(40):
            sx = _rand_seq(rng, rng.randrange(30, 700))
            sy = _evolve(rng, sx) or "C"
            anchors, x, y = [], -1, -1
            while True:
                x += rng.randrange(1, 5)
                y += rng.randrange(1, 5)
                if x >= len(sx) or y >= len(sy):
                    break
                anchors.append((x, y, exp))
            probs.append((sx, sy, anchors))
            raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
        kw = dict(diagonalExpansion=exp, minDiagsBetweenTraceBack=rng.randrange(60, 300), traceBackDiagonals=rng.randrange(5, 40),
                  splitMatrixBiggerThanThis=rng.choice([10, 50, 10 ** 12]))
        monkeypatch.setenv("CPECAN_PACKED", "2")
        packed, st_p = _run_batch(mtype, probs, raggeds, **kw)
        monkeypatch.setenv("CPECAN_PACKED", "0")
        sweep, st_s = _run_batch(mtype, probs, raggeds, **kw)
        assert st_p.cells == st_s.cells
        for a, b in zip(packed, sweep):
            assert a.shape == b.shape and (a == b).all()


def test_packed_split_classes_equal_whole_regions(monkeypatch):
    """Round 4: a packed class as two launches (cpk_packed.inl MODE: every forward sweep into a ring of the region's own,
    then one queue item per region and traceback segment, G items to a wave).  Forced on and off (CPECAN_PACKED_SPLIT) over
    all three group widths and both model families -- random anchors with several short traceback segments per region,
    ragged ends, split rectangles, a realign-style sample whose long alignments have a dozen segments, a threshold of zero
    (the per-segment slices overflow and the batch re-runs), wide regions riding along -- the lists must be identical
    triple for triple, and equal to the oracle's."""
    from cpecan_amd.workload import make_realign_batch
    rng = random.Random(2024)
    cases = []
    for mtype, exp in ((0, 2), (2, 6), (1, 14), (3, 26)):
        probs, raggeds = [], []
        for _ in range(40):
            sx = _rand_seq(rng, rng.randrange(1, 900))
            sy = _evolve(rng, sx) or "C"
            anchors, x, y = [], -1, -1
            while True:
                x += rng.randrange(1, 5)
                y += rng.randrange(1, 5)
                if x >= len(sx) or y >= len(sy):
                    break
                anchors.append((x, y, exp))
            probs.append((sx, sy, anchors))
            raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
        probs += [(_rand_seq(rng, 120), _rand_seq(rng, 130), [])] * 2  # wide: the sweep kernel, beside the packed classes
        raggeds += [(False, False)] * 2
        tbd = rng.randrange(5, 40)
        cases.append((mtype, probs, raggeds, dict(diagonalExpansion=exp, minDiagsBetweenTraceBack=tbd + rng.randrange(20, 200),
                                                   traceBackDiagonals=tbd, splitMatrixBiggerThanThis=rng.choice([10, 50, 10 ** 12]))))
    realign = make_realign_batch(4, 60, 100, 5000, 4)
    cases.append((0, realign, [(True, True)] * len(realign), dict(diagonalExpansion=4, splitMatrixBiggerThanThis=10,
                                                                  minDiagsBetweenTraceBack=1000, traceBackDiagonals=40)))
    cases.append((2, realign[:20], [(True, False)] * 20, dict(diagonalExpansion=4, threshold=0.0, minDiagsBetweenTraceBack=300,
                                                              traceBackDiagonals=20)))
    monkeypatch.setenv("CPECAN_PACKED", "2")
    for mtype, probs, raggeds, kw in cases:
        monkeypatch.setenv("CPECAN_PACKED_SPLIT", "0")
        whole, st0 = _run_batch(mtype, probs, raggeds, **kw)
        monkeypatch.setenv("CPECAN_PACKED_SPLIT", "1")
        split, st1 = _run_batch(mtype, probs, raggeds, **kw)
        assert st1.cells == st0.cells and st1.regions == st0.regions
        for a, b in zip(split, whole):
            assert a.shape == b.shape and (a == b).all()
        om, op = ob.model(mtype), ob.params(**kw)
        for i in range(0, len(probs), 7):
            sx, sy, an = probs[i]
            rl, rr = raggeds[i]
            assert_pairs_match(split[i], ob.aligned_pairs(om, sx, sy, an, op, rl, rr), threshold=op.threshold)
    # rings of whole regions are given up first when they do not fit the share of the device they may take: the split parts
    # fall back to whole regions (two launches of the whole-region kernel over the two parts of the class)
    mtype, probs, raggeds, kw = cases[4]
    monkeypatch.setenv("CPECAN_PACKED_SPLIT_FROM", "1500")
    monkeypatch.delenv("CPECAN_PACKED_SPLIT")
    monkeypatch.setenv("CPECAN_SPLIT_BUDGET_FRAC", "1e-7")
    back, st5 = _run_batch(mtype, probs, raggeds, **kw)
    monkeypatch.delenv("CPECAN_SPLIT_BUDGET_FRAC")
    cut, st6 = _run_batch(mtype, probs, raggeds, **kw)
    monkeypatch.setenv("CPECAN_PACKED_SPLIT", "0")
    ref5, _ = _run_batch(mtype, probs, raggeds, **kw)
    assert st5.deviceBytes < st6.deviceBytes
    for a, b, c in zip(back, cut, ref5):
        assert a.shape == c.shape and (a == c).all() and b.shape == c.shape and (b == c).all()
    monkeypatch.delenv("CPECAN_PACKED_SPLIT_FROM")
    # the default choice: a batch whose longest region is what a launch of whole regions waits for goes split by itself
    monkeypatch.delenv("CPECAN_PACKED_SPLIT")
    monkeypatch.delenv("CPECAN_PACKED")
    big = make_realign_batch(4, 400, 100, 5000, 4)
    kw = dict(diagonalExpansion=4, splitMatrixBiggerThanThis=10, minDiagsBetweenTraceBack=1000, traceBackDiagonals=40)
    auto, st2 = _run_batch(0, big, [(True, True)] * len(big), **kw)
    monkeypatch.setenv("CPECAN_PACKED_SPLIT", "0")
    ref, st3 = _run_batch(0, big, [(True, True)] * len(big), **kw)
    for a, b in zip(auto, ref):
        assert a.shape == b.shape and (a == b).all()


def test_packed_kernel_indel_emitter(monkeypatch):
    """the indel emitter (diagonalCalculationPosteriorProbs, pairwiseAligner.c:691-733 -- what
    getShiftedMEAAlignment :1764-1790 needs) on narrow bands through the packed kernel: the traceback parks B of the emitted
    cells and a pass behind the totals writes the three lists.  All three group widths, both model families, per-anchor
    expansions, split rectangles, short schedules, a realign-style sample: list for list what one wave per region gives
    (CPECAN_PACKED=0) -- bit for bit -- and what the oracle gives."""
    from cpecan_amd.workload import make_realign_batch
    rng = random.Random(321)
    cases = []
    for mtype, exp in ((0, 2), (2, 6), (1, 14), (3, 26)):
        probs, raggeds = [], []
        for _ in range(36):
            sx = _rand_seq(rng, rng.randrange(1, 500))
            sy = _evolve(rng, sx) or "C"
            anchors, x, y = [], -1, -1
            while True:
                x += rng.randrange(1, 5)
                y += rng.randrange(1, 5)
                if x >= len(sx) or y >= len(sy):
                    break
                anchors.append((x, y, exp))
            probs.append((sx, sy, anchors))
            raggeds.append((rng.random() > 0.5, rng.random() > 0.5))
        probs += [("A", "A", []), ("ACGTAC", "", []), ("", "GGT", [])]
        raggeds += [(False, False), (False, True), (True, True)]
        cases.append((mtype, probs, raggeds, dict(diagonalExpansion=exp, minDiagsBetweenTraceBack=rng.randrange(40, 200),
                                                  traceBackDiagonals=rng.randrange(3, 30),
                                                  splitMatrixBiggerThanThis=rng.choice([10, 50, 10 ** 12]))))
    sample = make_realign_batch(4, 40, 100, 2500, 4)
    cases.append((0, sample, [(True, True)] * len(sample), dict(diagonalExpansion=4, splitMatrixBiggerThanThis=10)))
    dyn = [(sx, sy, [(x, y, 2 * ((x * 7 + y) % 9)) for x, y, _ in a]) for sx, sy, a in cases[0][1]]
    cases.append((0, dyn, cases[0][2], dict(dynamicAnchorExpansion=1, minDiagsBetweenTraceBack=90, traceBackDiagonals=12)))

    def run(mtype, probs, raggeds, pkw):
        p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
        with api.Batch(_sm(mtype), p, emit=api.EMIT_INDEL) as b:
            for (sx, sy, a), (rl, rr) in zip(probs, raggeds):
                b.add(sx, sy, a, rl, rr)
            b.upload()
            b.run()
            b.download()
            return [[b.result(i, which).copy() for which in range(3)] for i in range(len(probs))], b.stats()

    for mtype, probs, raggeds, pkw in cases:
        monkeypatch.setenv("CPECAN_PACKED", "2")
        packed, st_p = run(mtype, probs, raggeds, pkw)
        monkeypatch.setenv("CPECAN_PACKED", "0")
        sweep, st_s = run(mtype, probs, raggeds, pkw)
        assert st_p.cells == st_s.cells and st_p.pairs == st_s.pairs
        om, op = ob.model(mtype), ob.params(**pkw)
        for i, (got, ref) in enumerate(zip(packed, sweep)):
            for which in range(3):
                assert got[which].shape == ref[which].shape and (got[which] == ref[which]).all(), (i, which)
            if i % 5 == 0:
                (sx, sy, a), (rl, rr) = probs[i], raggeds[i]
                want = ob.aligned_pairs_with_indels(om, sx, sy, a, op, rl, rr)
                for which in range(3):
                    assert_pairs_match(got[which], want[which], threshold=op.threshold)


def test_packed_kernel_degenerate_regions(force_packed):
    """One-base and one-sided problems, anchors on the very first / last base, through the packed kernel."""
    probs = [("A", "A", []), ("A", "ACGT", []), ("ACGTAC", "", []), ("", "GGT", []), ("ACGT", "ACGT", [(0, 0, 2), (3, 3, 2)]),
             ("ACGTACGTAC", "ACGTTACGTAC", [(0, 0, 4)]), ("N", "N", []), ("acgtn", "ACGTN", [(2, 2, 0)])]
    raggeds = [(False, False), (True, False), (False, True), (True, True)] * 2
    for mtype in (0, 2):
        _check_batch(mtype, probs, raggeds, diagonalExpansion=4)
        _check_batch(mtype, probs, raggeds, diagonalExpansion=0, threshold=0.0)


def test_packed_kernel_output_overflow_rerun(force_packed):
    """threshold ~0 on 13-cell-wide bands emits more pairs than the default slices hold: exact re-run, packed kernel."""
    problems = [make_pair(8, i, 200 + 30 * i, 12, anchor_every=3) for i in range(6)]
    kw = dict(diagonalExpansion=12, threshold=1e-9)
    got, st = _run_batch(0, problems, **kw)
    assert st.launches >= 2
    for (sx, sy, a), g in zip(problems, got):
        assert_pairs_match(g, ob.aligned_pairs(ob.model(0), sx, sy, a, ob.params(**kw)), threshold=1e-9)


@pytest.mark.parametrize("mtype", [0, 2])
def test_packed_kernel_expectations(force_packed, mtype):
    """The EM E-step as cPecanRealign runs it (--outputExpectations, cPecanRealign.c:530-534): dense anchors, expansion 4,
    ragged ends, split at 10 -- narrow bands, so the packed kernel computes the expectations."""
    from cpecan_amd.workload import make_realign_batch
    problems = make_realign_batch(6, 40, 100, 2600, 4) + [("ACGTNACGT", "ACGTACGT", [(1, 1, 4)]), ("A", "A", [])]
    kw = dict(diagonalExpansion=4, splitMatrixBiggerThanThis=10)
    p = api.pairwiseAlignmentBandingParameters_construct(**kw)
    op = ob.params(**kw)
    sM, om = _sm(mtype), ob.model(mtype)
    got = api.hmm_constructEmpty(1e-12, mtype)
    with api.Batch(sM, p, emit=api.EMIT_EXPECT) as b:
        for sx, sy, a in problems:
            b.add(sx, sy, a, True, True)
        b.upload()
        b.run()
        b.download()
        b.expectations(got)
    want = ob.hmm(mtype, 1e-12)
    for sx, sy, a in problems:
        ob.expectations(om, want, sx, sy, a, op, True, True)
    _assert_hmm_close(got, want, 5 if mtype < 2 else 3)


# ---- per-cell log-space values: sharper than any posterior (they see every logAdd of both sweeps) ----
@pytest.mark.parametrize("form", ["whole", "split_abs", "fused_abs", "split_dense_rows"])
@pytest.mark.parametrize("case", ["tiny5", "tiny3", "full200", "A_1kb", "B_2kb", "short_tracebacks", "asym_ragged"])
def test_cell_values_and_totals_match_oracle(case, form, monkeypatch):
    """F.match + B.match of every emitted cell and the total probability used on every emitted diagonal (the debug
    buffers of the sweep kernel) against the oracle's trace of the same problem: equal to LOG_TOL (tests/parity.py), i.e.
    ~1e-12 relative -- seven orders inside the north star's 1e-5.  Multi-segment tracebacks, both state counts, ragged ends.
    form: one wave per region; the split forms (tracebacks as queue items: two launches / one launch), whose sweeps index
    the rolling rows by absolute position (round 3); the two-launch form with the rows indexed by rank (CPECAN_ABS=0)."""
    from parity import LOG_TOL
    if form != "whole" and case in ("tiny5", "tiny3", "full200"):
        pytest.skip("single-segment problems run one wave per region")
    monkeypatch.setenv("CPECAN_SPLIT", {"whole": "0", "split_abs": "1", "fused_abs": "2", "split_dense_rows": "1"}[form])
    monkeypatch.setenv("CPECAN_ABS", "0" if form == "split_dense_rows" else "1")
    rl = rr = False
    if case == "tiny5":
        mtype, (sx, sy, a), pkw = 0, ("AGCG", "AGTTCG", ()), dict(threshold=0.2)
    elif case == "tiny3":
        mtype, (sx, sy, a), pkw = 2, ("AGCG", "AGTTCG", ()), dict(threshold=0.2)
    elif case == "full200":
        mtype, (sx, sy, a), pkw = 0, make_pair(1, 0, 200, 0), dict(diagonalExpansion=20)
        a = ()
    elif case == "A_1kb":
        mtype, (sx, sy, a), pkw = 2, make_pair(2, 0, 1000, 50), dict(diagonalExpansion=50)
    elif case == "B_2kb":
        mtype, (sx, sy, a), pkw = 0, make_pair(3, 0, 2000, 100), dict(diagonalExpansion=100)
    elif case == "short_tracebacks":
        mtype, (sx, sy, a), pkw = 0, make_pair(3, 1, 600, 10), dict(diagonalExpansion=10, minDiagsBetweenTraceBack=50,
                                                                  traceBackDiagonals=7)
    else:
        mtype, (sx, sy, a), pkw = 1, make_pair(3, 2, 1500, 30), dict(diagonalExpansion=30)
        rl = rr = True
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
    want, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**pkw), rl, rr)
    with api.Batch(_sm(mtype), p, debug=True) as b:
        b.add(sx, sy, a, rl, rr)
        b.upload()
        b.run()
        b.download()
        got = b.result(0)
        fb, tot = b.debug_fetch(0, tr["n_cells"], tr["n_diagonals"])
    assert_pairs_match(got, want, threshold=p.threshold)
    ofb, otot = tr["fb_match"], tr["total_used"]
    m = ~np.isnan(ofb)
    inf = np.isinf(ofb[m])
    assert np.array_equal(np.isinf(fb[m]), inf) and np.array_equal(fb[m][inf], ofb[m][inf])
    scale = np.maximum(1.0, np.abs(ofb[m][~inf]))
    assert np.all(np.abs(fb[m][~inf] - ofb[m][~inf]) <= LOG_TOL * scale), float(np.max(np.abs(fb[m][~inf] - ofb[m][~inf])))
    mt = ~np.isnan(otot)
    assert mt.any()
    assert np.all(np.abs(tot[mt] - otot[mt]) <= LOG_TOL * np.maximum(1.0, np.abs(otot[mt]))), float(np.max(np.abs(tot[mt] - otot[mt])))


@pytest.mark.parametrize("second_pass", [False, True])
def test_expectation_emitter_cell_values_match_oracle(second_pass, monkeypatch):
    """The same debug buffers under the expectation emitter, whose traceback is a function of its own when the events are
    formed inside it (Sweep::tracebackExpect: forward rows in LDS, stores deferred by a diagonal) -- one and two groups per
    diagonal, several segments -- and under its second-pass form."""
    from parity import LOG_TOL
    monkeypatch.setenv("CPECAN_EXP_INSWEEP", "0" if second_pass else "2")
    for mtype, (sx, sy, a), pkw in ((0, make_pair(3, 1, 600, 10), dict(diagonalExpansion=10, minDiagsBetweenTraceBack=50, traceBackDiagonals=7)),
                                    (2, make_pair(2, 0, 1000, 50), dict(diagonalExpansion=50)),
                                    (0, make_pair(5, 0, 1200, 30), dict(diagonalExpansion=30))):
        p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
        _, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**pkw), False, False)
        with api.Batch(_sm(mtype), p, emit=api.EMIT_EXPECT, debug=True) as b:
            b.add(sx, sy, a, False, False)
            b.upload()
            b.run()
            b.download()
            fb, tot = b.debug_fetch(0, tr["n_cells"], tr["n_diagonals"])
        ofb, otot = tr["fb_match"], tr["total_used"]
        m = ~np.isnan(ofb) & ~np.isinf(ofb)
        assert np.all(np.abs(fb[m] - ofb[m]) <= LOG_TOL * np.maximum(1.0, np.abs(ofb[m]))), float(np.max(np.abs(fb[m] - ofb[m])))
        mt = ~np.isnan(otot)
        assert mt.any() and np.all(np.abs(tot[mt] - otot[mt]) <= LOG_TOL * np.maximum(1.0, np.abs(otot[mt])))


def test_one_launch_form_keeps_spare_slots_only_beside_a_live_batch(monkeypatch):
    """The one-launch form of a split class fills every wave slot of the chip when the batch has the device to itself and
    leaves one slot in every eighth CU free when another batch of the process has run there and is still alive (its list
    gather and the next batch's table build need somewhere to run: DESIGN.md section 5).  Same lists either way."""
    import gc
    import torch
    monkeypatch.delenv("CPECAN_SPLIT", raising=False)
    gc.collect()  # batches that earlier tests left to the collector count as alive until they are destroyed
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    probs = [make_pair(4, i, 2000, 100) for i in range(460)]  # regions + segments > wave slots (ten per CU since round 4)
    sm = api.stateMachine5_construct()
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=100)
    arr, cnt, keep = api.Batch.prepare_problems(probs)

    def one():
        b = api.Batch(sm, p)
        b.add_prepared(arr, cnt)
        b.upload()
        b.run()
        b.download()
        return b

    alone = one()
    beside = one()                       # planned while `alone` is alive
    w_alone, w_beside = alone.stats().wavesPerLaunch, beside.stats().wavesPerLaunch
    lists_alone = [alone.result(i) for i in range(cnt)]
    lists_beside = [beside.result(i) for i in range(cnt)]
    alone.close()
    beside.close()
    again = one()                        # nothing alive any more
    w_again = again.stats().wavesPerLaunch
    again.close()
    assert w_alone == w_again and w_alone - w_beside == cus // 8, (w_alone, w_beside, w_again, cus)
    for x, y in zip(lists_alone, lists_beside):
        assert np.array_equal(x, y)


# ---- batches as a pipeline: every batch on streams and events of its own (SURVEY 8d's host-to-host clock) ----
def test_pipelined_batches_equal_unpipelined_ones():
    """Two batches in flight from one host thread -- batch k+1 is packed, planned and uploaded and batch k-1 is gathered and
    downloaded while the sweep kernel of batch k runs -- give, list for list, what the same batches give one after the
    other; and so do batches driven from two host threads at once.  (bench.py's `value_e2e` is measured this way.)"""
    import threading
    rng = random.Random(907)
    pkw = dict(diagonalExpansion=20, splitMatrixBiggerThanThis=900)
    jobs = [_fuzz_problems(rng, 60, 20) for _ in range(5)]
    jobs.append(([make_pair(3, i, 2000, 100) for i in range(3)], [(False, False)] * 3))  # multi-segment regions too
    serial = [_run_batch(0, probs, raggeds, **pkw)[0] for probs, raggeds in jobs]
    p = api.pairwiseAlignmentBandingParameters_construct(**pkw)

    def start(k):
        probs, raggeds = jobs[k]
        b = api.Batch(_sm(0), p)
        b.add_many([(sx, sy, a, rl, rr) for (sx, sy, a), (rl, rr) in zip(probs, raggeds)])
        b.upload()
        b.run()
        return b

    def finish(k, b, into):
        b.download()
        into[k] = [b.result(i) for i in range(len(jobs[k][0]))]
        b.close()

    piped = [None] * len(jobs)
    prev = start(0)
    for k in range(1, len(jobs)):
        cur = start(k)          # while batch k-1 is still running or waiting to be read
        finish(k - 1, prev, piped)
        prev = cur
    finish(len(jobs) - 1, prev, piped)
    threaded = [None] * len(jobs)

    def worker(t):
        for k in range(t, len(jobs), 2):
            finish(k, start(k), threaded)
    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    # the download on the batch's own helper thread (cpecan_batch_download_begin / _end): begun right behind the launch,
    # ended one batch later -- the caller packs and uploads the next batch in between
    helped = [None] * len(jobs)

    def end(k, b):
        b.download_end()
        helped[k] = [b.result(i) for i in range(len(jobs[k][0]))]
        b.close()

    prev = start(0)
    prev.download_begin()
    with pytest.raises(api.CpecanError):
        prev.download_begin()  # one download at a time per batch
    # while the helper thread rewrites the batch, every other entry point refuses it (CPECAN_ESTATE) instead
    # of racing with it
    for refused in (prev.download, lambda: prev.result(0), prev.run, prev.stats):
        with pytest.raises(api.CpecanError):
            refused()
    for k in range(1, len(jobs)):
        cur = start(k)
        cur.download_begin()
        end(k - 1, prev)
        prev = cur
    end(len(jobs) - 1, prev)
    for name, got in (("pipelined", piped), ("two host threads", threaded), ("helper-thread downloads", helped)):
        for k, (g, w) in enumerate(zip(got, serial)):
            assert g is not None and len(g) == len(w), (name, k)
            for i, (a, b) in enumerate(zip(g, w)):
                assert np.array_equal(a, b), (name, "job", k, "problem", i, len(a), len(b))


def test_table_built_by_a_wave_per_region_equals_the_serial_one(monkeypatch):
    """Round 4: the per-diagonal table (and the position chains of the absolute-position sweeps) of a split class's regions
    is built by one WAVE per region -- every lane a chunk of the diagonals: band iterator set by a binary search over the
    anchors, offsets by a wave scan, position chains replayed from the nearest re-base point -- instead of one thread
    (CPECAN_TABLE_WAVE=0).  Same lists, bit for bit, in both split forms: fixed expansions (absolute positions), per-anchor
    expansions (rank-indexed rows), no anchors at all, regions shorter than a wave has lanes, split rectangles."""
    rng = random.Random(4040)
    cases = []
    cases.append((0, [make_pair(3, i, 2000, 100) for i in range(5)] + [make_pair(2, i, 700, 30) for i in range(5)], None,
                  dict(diagonalExpansion=100)))
    cases.append((2, [make_pair(2, i, 1000, 50) for i in range(10)], None, dict(diagonalExpansion=50)))
    fz, rg = _fuzz_problems(rng, 40, 20)
    cases.append((0, fz, rg, dict(diagonalExpansion=20, minDiagsBetweenTraceBack=60, traceBackDiagonals=7, splitMatrixBiggerThanThis=900)))
    fz2, rg2 = _fuzz_problems(rng, 30, 12)
    dyn = [(sx, sy, [(x, y, 2 * ((3 * x + y) % 11)) for x, y, *_ in a]) for sx, sy, a in fz2]
    cases.append((0, dyn, rg2, dict(dynamicAnchorExpansion=1, minDiagsBetweenTraceBack=80, traceBackDiagonals=9)))
    cases.append((2, [("ACGTTGCA" * 40, "ACGTTGCA" * 41, ()), ("A", "C", ()), ("ACGT", "", ()), ("AC" * 30, "AC" * 29, [(5, 5, 4)])], None,
                  dict(diagonalExpansion=4, minDiagsBetweenTraceBack=50, traceBackDiagonals=3)))
    for mtype, problems, raggeds, pkw in cases:
        for form in ("1", "2"):
            monkeypatch.setenv("CPECAN_SPLIT", form)
            monkeypatch.setenv("CPECAN_TABLE_WAVE", "0")
            serial, st0 = _run_batch(mtype, problems, raggeds, **pkw)
            monkeypatch.delenv("CPECAN_TABLE_WAVE")
            wave, st1 = _run_batch(mtype, problems, raggeds, **pkw)
            assert (st1.cells, st1.pairs, st1.launchForm) == (st0.cells, st0.pairs, st0.launchForm)
            for i, (a, b) in enumerate(zip(wave, serial)):
                assert np.array_equal(a, b), (form, i)
        om, op = ob.model(mtype), ob.params(**pkw)
        for i in range(0, len(problems), 4):
            sx, sy, a = problems[i]
            rl, rr = raggeds[i] if raggeds else (False, False)
            assert_pairs_match(wave[i], ob.aligned_pairs(om, sx, sy, a, op, rl, rr), threshold=op.threshold)


def test_one_launch_form_times_out_into_two_launches(monkeypatch):
    """an item of the one-launch form that gives up waiting for its region's forward values (here: after a
    single poll, CPECAN_FUSED_SPIN=1) is reported by the launch, and the download runs the class again as two launches
    instead of failing -- same lists as one wave per region."""
    probs = [make_pair(4, i, 2000, 60) for i in range(24)]
    monkeypatch.setenv("CPECAN_SPLIT", "0")
    whole, st0 = _run_batch(0, probs, diagonalExpansion=60)
    monkeypatch.setenv("CPECAN_SPLIT", "2")
    monkeypatch.setenv("CPECAN_FUSED_SPIN", "1")
    fused, st1 = _run_batch(0, probs, diagonalExpansion=60)
    assert st1.launches >= 1 and st1.cells == st0.cells
    for a, b in zip(fused, whole):
        assert np.array_equal(a, b)


def test_cache_trim_gives_idle_blocks_back():
    """idle device / host blocks of destroyed batches can be returned to the driver (cpecan_cache_trim), and
    the library keeps working afterwards."""
    sx, sy, a = make_pair(3, 0, 600, 20)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=20)
    first = api.getAlignedPairsUsingAnchors(api.stateMachine5_construct(), sx, sy, a, p)
    freed = api.cache_trim(0)
    assert freed > 0  # the batch of the call above left its blocks in the cache
    assert api.cache_trim(-1) == 0  # nothing idle is left
    again = api.getAlignedPairsUsingAnchors(api.stateMachine5_construct(), sx, sy, a, p)
    assert np.array_equal(first, again)


def test_one_batch_at_a_time_does_not_stall():
    """a caller that runs one big batch at a time (create -> run -> download -> destroy: zero live
    batches between two of them) must not pay hipFree + hipMalloc of the batch's device blocks around every batch.
    Round 3 trimmed the device cache whenever the last live batch of a device was destroyed: the next 20+ GB batch
    waited seconds for its ring block.  The blocks now stay until the device has been idle for CPECAN_CACHE_IDLE_S
    (default 20 s) or cpecan_cache_trim() is called.  One warm-up iteration (the first hipMalloc of the process is what it
    is), then five timed ones: none may take more than twice the median; and the explicit trim still returns the blocks."""
    import time
    from cpecan_amd import workload
    cfg = workload.CONFIGS["B"]
    n = 3500
    problems = workload.config_problems("B", range(n))
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=cfg["expansion"])
    api.cache_trim(0)
    times, dev_bytes, first = [], 0, None
    for it in range(6):
        t0 = time.perf_counter()
        with api.Batch(_sm(0), p) as b:
            b.add_many(problems)
            b.upload()
            b.run()
            b.download()
            dev_bytes = b.stats().deviceBytes
            got = b.result(n - 1).copy()
        times.append(time.perf_counter() - t0)
        if first is None:
            first = got
        assert np.array_equal(first, got)
    assert dev_bytes >= 20e9, dev_bytes  # the headline launch form: per-region rings, ~19 MB per pair
    timed = sorted(times[1:])
    median = timed[len(timed) // 2]
    print("one batch at a time, %d config-B pairs, %.1f GB on the device: warm-up %.3f s, then %s (median %.3f s)"
          % (n, dev_bytes / 1e9, times[0], " ".join("%.3f" % t for t in times[1:]), median))
    assert max(times[1:]) <= 2.0 * median, times
    assert api.cache_trim(0) >= 20e9  # ... and the blocks were idle in the cache, the caller's to give back


def test_entry_points_leave_the_callers_current_device_alone():
    """a batch works on ITS device and restores the calling thread's current device (torch follows
    hipGetDevice); single-problem calls run on the caller's current device.  One GPU here: the guard must at least
    be a no-op that keeps device 0 current through every stage."""
    import torch
    assert torch.cuda.current_device() == 0
    sx, sy, a = make_pair(1, 0, 300, 20)
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=20)
    got = api.getAlignedPairsUsingAnchors(api.stateMachine5_construct(), sx, sy, a, p)
    assert len(got) > 0 and torch.cuda.current_device() == 0
    x = torch.ones(4, device="cuda")  # still allocates on the device the caller chose
    assert x.device.index == 0


# ---- the cases the reference's tests hold beyond geometry, through the HIP path ----
def test_getAlignedPairsWithRaggedEnds_exact_outcome_gpu():
    """tests/pairwiseAlignerTest.c:676-715 through getAlignedPairs + filterPairwiseAlignmentToMakePairsOrdered on the GPU:
    exactly the 100 pairs (x, x + 100), 120 seeded trials in one batch (ragged priors + ordered filter, exact outcome),
    and list for list what the oracle gives."""
    import reference_cases as rc
    p = api.pairwiseAlignmentBandingParameters_construct()
    trials = [rc.ragged_ends_trial(t) for t in range(120)]
    with api.Batch(api.stateMachine5_construct(), p) as b:
        b.add_many([(sx, sy, (), True, True) for sx, sy in trials])
        b.set_post(api.POST_ORDERED, matchGamma=0.2)
        b.upload()
        b.run()
        b.download()
        om, op = ob.model(ob.FIVE_STATE), ob.params()
        for i, (sx, sy) in enumerate(trials):
            out = b.result(i, 3)
            assert len(out) == 100 and all(int(y) == int(x) + 100 for _, x, y in out), i
            if i < 12:
                want = ob.aligned_pairs(om, sx, sy, (), op, True, True)
                assert_pairs_match(b.result(i), want, threshold=p.threshold)
    # the single-call entry points give the same
    sx, sy = trials[0]
    pairs = api.getAlignedPairsUsingAnchors(api.stateMachine5_construct(), sx, sy, (), p, True, True)
    out = api.filterPairwiseAlignmentToMakePairsOrdered(pairs, sx, sy, 0.2)
    assert len(out) == 100 and all(int(y) == int(x) + 100 for _, x, y in out)


def test_trained_hmm_of_the_reference_through_the_gpu():
    """cPecanEmTest.py:112-113's trained five-state-asymmetric HMM: hmm_loadFromFile -> hmm_getStateMachine -> alignments
    and expectations on the GPU against the oracle with the model built from the same numbers."""
    import reference_cases as rc
    mtype, T, lik, E = rc.trained_hmm_numbers()
    sm = api.hmm_getStateMachine(api.hmm_loadFromFile(rc.TRAINED_HMM))
    oh = ob.hmm(ob.FIVE_STATE_ASYM, 0.0)
    for i, v in enumerate(T):
        oh.T[i] = v
    for i, v in enumerate(E):
        oh.E[i] = v
    om = ob.model_from_hmm(oh)
    kw = dict(diagonalExpansion=20)
    p, op = api.pairwiseAlignmentBandingParameters_construct(**kw), ob.params(**kw)
    probs = [make_pair(31, i, 700, 20) for i in range(6)]
    for sx, sy, a in probs:
        got = api.getAlignedPairsUsingAnchors(sm, sx, sy, a, p, True, False)
        assert len(got) > 0
        assert_pairs_match(got, ob.aligned_pairs(om, sx, sy, a, op, True, False), threshold=p.threshold)
    acc, oacc = api.hmm_constructEmpty(0.0, api.fiveStateAsymmetric), ob.hmm(ob.FIVE_STATE_ASYM, 0.0)
    for sx, sy, a in probs[:3]:
        api.getExpectationsUsingAnchors(sm, acc, sx, sy, a, p)
        ob.expectations(om, oacc, sx, sy, a, op)
    _assert_hmm_close(acc, oacc, 5)


def test_encode_human_chimp_full_length_gpu():
    """tests/pairwiseAlignerLongTest.c's ~57 kb human / chimp ENCODE pair at full length through the HIP path: 115 k
    anti-diagonals, ~115 traceback segments in one region; every pair against the oracle, and sensitivity / specificity
    against the embedded reference alignment as the reference's test logs them (:100-108; the 0.99 bars are ours)."""
    import reference_cases as rc
    sx, sy, anchors, true_pairs = rc.encode_human_chimp()
    kw = dict(diagonalExpansion=20)
    p = api.pairwiseAlignmentBandingParameters_construct(**kw)
    got = api.getAlignedPairsUsingAnchors(api.stateMachine5_construct(), sx, sy, anchors, p)
    want = ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, anchors, ob.params(**kw))
    assert len(want) > 56000
    assert_pairs_match(got, want, threshold=p.threshold)
    out = api.filterPairwiseAlignmentToMakePairsOrdered(got, sx, sy, 0.5)
    sens, spec = rc.sensitivity_specificity(out, true_pairs)
    print("ENCODE human/chimp through the HIP path: %d pairs, sensitivity %.5f, specificity %.5f" % (len(out), sens, spec))
    assert sens > 0.99 and spec > 0.99
    # split into regions at large anchor gaps (getSplitPoints): same lists
    p2 = api.pairwiseAlignmentBandingParameters_construct(splitMatrixBiggerThanThis=100, **kw)
    got2 = api.getAlignedPairsUsingAnchors(api.stateMachine5_construct(), sx, sy, anchors, p2)
    want2 = ob.aligned_pairs(ob.model(ob.FIVE_STATE), sx, sy, anchors, ob.params(splitMatrixBiggerThanThis=100, **kw))
    assert_pairs_match(got2, want2, threshold=p.threshold)


@pytest.mark.parametrize("species", ["mouse", "dog"])
def test_encode_human_mouse_and_dog_full_length_gpu(species):
    """tests/pairwiseAlignerLongTest.c:128-134: the divergent human / mouse and human / dog ENCODE pairs at full length
    through the HIP path.  One region of ~90-110 k anti-diagonals whose band alternates between 40-cell parallelograms
    and full rectangles of up to 1947 x 1329 cells (diagonals of > 1300 cells: the wide classes), then the same problem
    split at the large gaps (getSplitPoints, many small regions): every pair against the oracle."""
    import reference_cases as rc
    sx, sy, anchors, true_pairs = rc.encode_human_other(species)
    sm, om = api.stateMachine5_construct(), ob.model(ob.FIVE_STATE)
    for kw in (dict(diagonalExpansion=20), dict(diagonalExpansion=20, splitMatrixBiggerThanThis=500)):
        p = api.pairwiseAlignmentBandingParameters_construct(**kw)
        got = api.getAlignedPairsUsingAnchors(sm, sx, sy, anchors, p)
        want = ob.aligned_pairs(om, sx, sy, anchors, ob.params(**kw))
        assert len(want) > 25000
        assert_pairs_match(got, want, threshold=p.threshold)
        if len(kw) == 1:
            out = api.filterPairwiseAlignmentToMakePairsOrdered(got, sx, sy, 0.5)
            sens, spec = rc.sensitivity_specificity(out, true_pairs)
            print("ENCODE human/%s through the HIP path: %d pairs, sensitivity %.5f, specificity %.5f" % (species, len(out), sens, spec))


# ---- split classes: the tracebacks of a region as queue items of their own (fills the chip when regions < wave slots) ----
def test_split_classes_equal_whole_region_waves(monkeypatch):
    """A class with fewer regions than the chip has wave slots runs as two launches: forward sweeps of whole regions into
    per-region rings, then one queue item per (region, traceback segment).  Forced on (CPECAN_SPLIT=1) over a mixed batch
    -- multi-segment 2 kb pairs, short-schedule pairs, single-segment and empty regions, split rectangles, thresholds down
    to 0 (every cell emitted: the per-segment output slices overflow and the batch re-runs) -- it must give, list for
    list, what one wave per region gives (CPECAN_SPLIT=0), and the oracle's lists."""
    rng = random.Random(1207)
    cases = []
    probs = [make_pair(3, i, 2000, 100) for i in range(6)] + [make_pair(2, i, 1000, 50) for i in range(6)]
    cases.append((0, probs, dict(diagonalExpansion=100)))
    cases.append((2, [make_pair(2, i, 1000, 50) for i in range(12)], dict(diagonalExpansion=50)))
    fz, rg = _fuzz_problems(rng, 50, 20)
    cases.append((0, fz, dict(diagonalExpansion=20, minDiagsBetweenTraceBack=60, traceBackDiagonals=7, splitMatrixBiggerThanThis=900)))
    cases.append((0, [make_pair(7, i, 700, 20) for i in range(4)] + [("", "", ()), ("ACGT", "", ())],
                  dict(diagonalExpansion=20, minDiagsBetweenTraceBack=90, traceBackDiagonals=10, threshold=0.0)))
    # sparse anchors under a wide expansion: diagonals of > 256 cells, a class that goes to a TEAM of waves although its
    # regions would qualify for the absolute-position sweeps (round 4: the team's LDS was then sized for the symbol
    # windows of those sweeps while the team stages whole strings -- tools/soak_forms.py seed 41 round 33)
    cases.append((0, [make_pair(41, i, L, 100, anchor_every=400) for i, L in enumerate((1500, 2200, 900, 1800))],
                  dict(diagonalExpansion=100, threshold=0.0)))
    for mtype, problems, pkw in cases:
        monkeypatch.setenv("CPECAN_SPLIT", "0")
        whole, st0 = _run_batch(mtype, problems, **pkw)
        monkeypatch.setenv("CPECAN_SPLIT", "1")
        split, st1 = _run_batch(mtype, problems, **pkw)
        assert st1.cells == st0.cells
        for a, b in zip(split, whole):
            assert np.array_equal(a, b)
        # the same two launches with the rolling rows indexed by rank instead of absolute position (CPECAN_ABS=0)
        monkeypatch.setenv("CPECAN_ABS", "0")
        ranked, st3 = _run_batch(mtype, problems, **pkw)
        monkeypatch.delenv("CPECAN_ABS")
        assert st3.cells == st0.cells
        for a, b in zip(ranked, whole):
            assert np.array_equal(a, b)
        # ... and as ONE launch (CPECAN_SPLIT=2: regions and their traceback items in one queue, an item waits for its
        # region's forward wave to pass its segment)
        monkeypatch.setenv("CPECAN_SPLIT", "2")
        fused, st2 = _run_batch(mtype, problems, **pkw)
        assert st2.cells == st0.cells
        for a, b in zip(fused, whole):
            assert np.array_equal(a, b)
        om, op = ob.model(mtype), ob.params(**pkw)
        for i in range(0, len(problems), 5):
            sx, sy, an = problems[i]
            assert_pairs_match(split[i], ob.aligned_pairs(om, sx, sy, an, op), threshold=op.threshold)
    monkeypatch.delenv("CPECAN_SPLIT")
