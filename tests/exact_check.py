"""Run as a child process by tests/test_gpu_exact.py with CPECAN_LIB pointing at the diagnostic library
(`make -C cpecan_amd/csrc exact`: logAdd as the reference's operations one for one, impl/pairwiseAligner.c:287-307).
Every log-space value of the sweeps' debug buffers, every emitted triple, every forward probability must EQUAL the
oracle's -- tolerance zero.  Prints one line per case and exits non-zero on the first difference."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from cpecan_amd import api  # noqa: E402
from cpecan_amd.workload import make_pair  # noqa: E402
import oracle_binding as ob  # noqa: E402
import indel_cases as ic  # noqa: E402


def sm(mtype):
    return api.stateMachine5_construct(mtype) if mtype < 2 else api.stateMachine3_construct(mtype)


def main():
    assert "exact" in os.path.basename(api.LIB_PATH), api.LIB_PATH
    cases = [
        ("tiny5", 0, ("AGCG", "AGTTCG", ()), dict(threshold=0.2), False),
        ("tiny3", 2, ("AGCG", "AGTTCG", ()), dict(threshold=0.2), False),
        ("A_1kb", 2, make_pair(2, 0, 1000, 50), dict(diagonalExpansion=50), False),
        ("B_2kb", 0, make_pair(3, 0, 2000, 100), dict(diagonalExpansion=100), False),
        ("short_tracebacks", 0, make_pair(3, 1, 600, 10), dict(diagonalExpansion=10, minDiagsBetweenTraceBack=50,
                                                            traceBackDiagonals=7), False),
        ("asym_ragged", 1, make_pair(3, 2, 1500, 30), dict(diagonalExpansion=30), True),
    ]
    for name, mtype, (sx, sy, a), pkw, ragged in cases:
        p = api.pairwiseAlignmentBandingParameters_construct(**pkw)
        want, tr = ob.aligned_pairs_traced(ob.model(mtype), sx, sy, a, ob.params(**pkw), ragged, ragged)
        with api.Batch(sm(mtype), p, debug=True) as b:
            b.add(sx, sy, a, ragged, ragged)
            b.upload()
            b.run()
            b.download()
            got = b.result(0)
            fb, tot = b.debug_fetch(0, tr["n_cells"], tr["n_diagonals"])
        want = np.asarray(want, dtype=np.int64).reshape(-1, 3)
        assert np.array_equal(np.asarray(got, dtype=np.int64), want), (name, "triples differ")
        m = ~np.isnan(tr["fb_match"])
        assert np.array_equal(fb[m], tr["fb_match"][m]), (name, "F.match + B.match differs",
                                                          float(np.nanmax(np.abs(fb[m] - tr["fb_match"][m]))))
        mt = ~np.isnan(tr["total_used"])
        assert mt.any() and np.array_equal(tot[mt], tr["total_used"][mt]), (name, "totals differ")
        print("exact: %s: %d triples, %d cells, %d totals equal" % (name, len(want), int(m.sum()), int(mt.sum())), flush=True)
    # the production forms of the same kernels (split classes, no debug buffers): a batch of config-B-shaped pairs
    probs = [make_pair(5, i, 2000, 100) for i in range(24)]
    p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=100)
    with api.Batch(sm(0), p) as b:
        b.add_many(probs)
        b.upload()
        b.run()
        b.download()
        for i, (sx, sy, a) in enumerate(probs):
            want = np.asarray(ob.aligned_pairs(ob.model(0), sx, sy, a, ob.params(diagonalExpansion=100)), dtype=np.int64).reshape(-1, 3)
            assert np.array_equal(np.asarray(b.result(i), dtype=np.int64), want), ("batch", i)
    print("exact: batch of %d config-B pairs: every triple equal" % len(probs), flush=True)
    # forward probabilities (pure logAdd arithmetic)
    for mtype in (0, 2):
        sx, sy, a = make_pair(6, mtype, 700, 40)
        p = api.pairwiseAlignmentBandingParameters_construct(diagonalExpansion=40)
        got = api.computeForwardProbability(sx, sy, a, p, sm(mtype), False, False)
        want = ob.forward_prob(ob.model(mtype), sx, sy, a, ob.params(diagonalExpansion=40), False, False)
        assert got == want, ("forward", mtype, got, want)
    # ... on wide diagonals (four 64-lane groups; 701 cells of five states, the widest that keep their rows in LDS) and on
    # the global-memory kernel (721 cells of five states, 1121 of three: over the LDS path's 64 KB), ragged ends
    p = api.pairwiseAlignmentBandingParameters_construct()
    for mtype, length, rl, rr in ((0, 200, True, False), (3, 200, False, True), (0, 700, False, True), (0, 720, True, True), (2, 1120, False, False)):
        sx, sy, _ = make_pair(7, mtype, length, 0)
        sy = (sy + b"A" * length)[:length]  # the widest diagonal has length + 1 cells
        got = api.computeForwardProbability(sx, sy, (), p, sm(mtype), rl, rr)
        want = ob.forward_prob(ob.model(mtype), sx, sy, (), ob.params(), rl, rr)
        assert got == want, ("forward", mtype, length, got, want)
    # the three lists of the indel emitter from each of its list passes, under models whose X and Y numbers differ: one
    # wave per region at a threshold that lists most cells, the packed kernel, the team of four waves
    edge = ic.edges_case("threeStateAsymmetric")
    one_wave = ic.Case("exact-65x65", edge.model, tuple(p for p in edge.problems if (len(p[0]), len(p[1])) == (65, 65))[1:2], dict(threshold=1e-4))
    packed = ic.packed_cases("trained", 1e-3)[1][1]
    packed = ic.Case("exact-packed", packed.model, packed.problems[:4], packed.pkw)
    for case, knob in ((one_wave, None), (packed, "2"), (ic.team_cases("fiveStateAsymmetric", 1e-3)[0][2], None)):
        if knob:
            os.environ["CPECAN_PACKED"] = knob
        with api.Batch(ic.model_pair(case.model)[0], api.pairwiseAlignmentBandingParameters_construct(**case.pkw), emit=api.EMIT_INDEL) as b:
            b.add_many(case.problems)
            b.upload()
            b.run()
            b.download()
            for i, want in enumerate(ic.oracle_lists(case)):
                for which in range(3):
                    assert np.array_equal(np.asarray(b.result(i, which), dtype=np.int64), want[which]), (case.name, i, which)
        os.environ.pop("CPECAN_PACKED", None)
        print("exact: indel lists of %s equal (%d entries)" % (case.name, sum(len(t) for ls in ic.oracle_lists(case) for t in ls)), flush=True)
    print("exact: forward probabilities equal", flush=True)


if __name__ == "__main__":
    main()
