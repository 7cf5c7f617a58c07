"""An independent definition of filterPairwiseAlignmentToMakePairsOrdered for two sequences, quadratic, with no frontier
and no staircase: what impl/multipleAligner.c:358-492 computes, stated as a rule over ALL chain ends.

The rule, from the reference's lines:
  * a pair takes part when  w / PROB_1 >= matchGamma  and  > 0  (:395); matchGamma is a float widened to double (:945);
  * the columns of X go in ascending order (:384) and every pair of a column is scored before any of them becomes a chain
    end (:389-410, then :412-435), so a pair's predecessor lies in a STRICTLY earlier column, at a y' < y (:402);
  * the reference asks its sorted set for the entry with the largest y' below y.  The set keeps strictly growing scores
    along y: an end leaves (or never enters) only for one that scores at least as much at a y no larger, and of two at the
    same y and score the later column stays (:419-427).  So that entry is the end that is maximal under
    (chain score, then smaller y, then later column) among all ends below y -- which is what this file evaluates, by
    looking at every earlier end;
  * the chain score is  score(predecessor) + w * 1.0  (:407), 0 for no predecessor;
  * the alignment is walked back from the last entry of the set (:441-445): the maximal end under the same order;
  * the list conversions (:621-651, :582) pop from the back three times: the chosen pairs leave in reverse input order.
The st_random() jitter of :145 is left out, as everywhere in this project.  Cells must be distinct (a repeated cell is
refused by the library).

Test infrastructure: numpy only, nothing of the device and nothing of the oracle.
"""
import numpy as np

PROB_1 = 10000000


def qualifying(pairs, match_gamma):
    """Indices of the pairs that take part, in list order."""
    g = float(np.float32(match_gamma))
    return [i for i, (w, _, _) in enumerate(pairs) if w / PROB_1 >= g and w / PROB_1 > 0.0]


def _best(mask, score, ys, xs):
    """Index of the end that is maximal under (score, smaller y, later column) among mask; -1 for none."""
    if not mask.any():
        return -1
    sel = mask & (score == score[mask].max())
    sel &= ys == ys[sel].min()
    sel &= xs == xs[sel].max()
    idx = np.flatnonzero(sel)
    assert len(idx) == 1, "a repeated cell"
    return int(idx[0])


def chain(pairs, match_gamma):
    """(q, pred, score, last): the qualifying indices, each one's predecessor as a position in q (-1: none), its chain
    score, and the position of the final end (-1: nothing takes part)."""
    q = qualifying(pairs, match_gamma)
    m = len(q)
    w = np.array([pairs[i][0] / PROB_1 for i in q], dtype=np.float64)
    xs = np.array([pairs[i][1] for i in q], dtype=np.int64)
    ys = np.array([pairs[i][2] for i in q], dtype=np.int64)
    score = np.zeros(m, dtype=np.float64)
    pred = np.full(m, -1, dtype=np.int64)
    for k in np.argsort(xs, kind="stable"):  # ascending columns; every end used below lies in an earlier one, so is scored
        p = _best((xs < xs[k]) & (ys < ys[k]), score, ys, xs)
        pred[k] = p
        score[k] = (score[p] if p >= 0 else 0.0) + w[k] * 1.0
    last = _best(np.ones(m, dtype=bool), score, ys, xs) if m else -1
    return q, pred, score, last


def filter_pairs_ordered(pairs, match_gamma):
    """The chosen pairs as (w, x, y) tuples, in reverse input order."""
    pairs = [tuple(int(v) for v in t) for t in pairs]
    q, pred, _, k = chain(pairs, match_gamma)
    chosen = set()
    while k >= 0:
        chosen.add(q[k])
        k = int(pred[k])
    return [pairs[i] for i in range(len(pairs) - 1, -1, -1) if i in chosen]
