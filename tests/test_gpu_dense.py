"""The dense rows of cpecan_amd.dense (cpk_dense.inl) against the oracle's trace, ob.aligned_pairs_traced, for cases (a)-(f) of
tests/dense_cases.py: the band and the cell offsets exactly; F over all states, F.match + B.match wherever the oracle recorded
it, and the totals used at parity.LOG_TOL, scaled as test_cell_values_and_totals_match_oracle scales it; infinities in the same
places.  Case (g): the inputs together in ONE object and one run give the same arrays, bit for bit, as run one at a time.
The exact library makes the same comparisons at tolerance zero: tests/dense_exact_check.py, one child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
from cpecan_amd import dense
from parity import LOG_TOL

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = os.path.join(os.path.dirname(HERE), "cpecan_amd", "libcpecan_hip_exact.so")


def _rows(c):
    return dense.forward_backward(dc.model_pair(c.model)[0], c.sx, c.sy, dc.anchors_of(c), dc.lib_params(c), c.ragged_left,
                                  c.ragged_right)


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_rows_match_the_oracle_trace(name):
    c = dc.case(name)
    print(dc.compare_with_oracle(c, _rows(c), LOG_TOL))


@pytest.mark.gpu
def test_b_next_is_the_row_the_straddle_term_used():
    """Bnext of a traceback is ITS backward row of tbFrom + 1, not the next traceback's (B of that diagonal): recompute the total
    used on tbFrom from F, B and Bnext on the host -- the oracle's fold, its logAdd -- and hold it against total_used."""
    import oracle_binding as ob
    c = dc.case("c_segments")
    r, om = _rows(c), dc.model_pair(c.model)[1]
    sym = lambda s, i: ob.symbol(chr(s[i - 1])) if i > 0 else 4  # noqa: E731
    assert len(r.segs) >= 5
    for k, (tb_prev, d_top, d) in enumerate(r.segs[:-1]):
        f = r.F[r.cell_off[d]:r.cell_off[d + 1]]
        b = r.B[r.cell_off[d]:r.cell_off[d + 1]]
        total = -np.inf
        for fc, bc in zip(f, b):
            t = fc[0] + bc[0]
            for s in range(1, 5):
                t = ob.log_add(t, fc[s] + bc[s])
            total = ob.log_add(total, t)
        nxt = r.b_next[r.b_next_off[k]:r.b_next_off[k + 1]]
        assert len(nxt) == r.diags[d + 1][1]
        assert not np.array_equal(nxt, r.B[r.cell_off[d + 1]:r.cell_off[d + 2]])  # the next traceback's values differ
        straddle = -np.inf
        to_match = [om.tr[i].tP for i in range(om.nTransitions) if om.tr[i].block == 1]
        assert len(to_match) == 5
        for j in range(len(nxt)):
            xmy = int(r.diags[d + 1][0]) + 2 * j
            kd = (xmy - int(r.diags[d - 1][0])) // 2
            m = -np.inf
            if 0 <= kd < r.diags[d - 1][1]:
                x, y = (d + 1 + xmy) // 2, (d + 1 - xmy) // 2
                e = om.matchEm[sym(c.sx, x) * 5 + sym(c.sy, y)]
                for s in range(5):
                    m = ob.log_add(m, r.F[r.cell_off[d - 1] + kd][s] + (e + to_match[s]))
            straddle = ob.log_add(straddle, m + nxt[j][0])
        total = ob.log_add(total, straddle)
        assert abs(total - r.total_used[d]) <= LOG_TOL * max(1.0, abs(total)), (k, total, r.total_used[d])


@pytest.mark.gpu
@pytest.mark.parametrize("config", dc.JOINT_CONFIGS)
def test_one_object_one_run_equals_one_at_a_time(config):
    """(g): offsets between problems.  Bit for bit, NaN for NaN."""
    cfg = dc.case(config)
    sm, p = dc.model_pair(cfg.model)[0], dc.lib_params(cfg)
    with dense.Dense(sm, p) as d:
        for i, c in enumerate(dc.cases()):
            assert d.add(c.sx, c.sy, dc.anchors_of(c), c.ragged_left, c.ragged_right) == i
        d.run()
        together = [d.rows(i) for i in range(d.n)]
    for c, got in zip(dc.cases(), together):
        alone = dense.forward_backward(sm, c.sx, c.sy, dc.anchors_of(c), p, c.ragged_left, c.ragged_right)
        for field, a, b in zip(got._fields, got, alone):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (config, c.name, field)
        if c.name == config:  # and that configuration's own case is the one the oracle comparison knows
            dc.compare_with_oracle(c, got, LOG_TOL)


@pytest.mark.gpu
def test_exact_build_gives_the_oracle_rows_bit_for_bit():
    assert os.path.exists(EXACT), "%s is missing: __graft_entry__.build() makes it (`make -C cpecan_amd/csrc exact`)" % EXACT
    env = dict(os.environ, CPECAN_LIB=EXACT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "dense_exact_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "dense rows equal" in r.stdout
