"""The preconditions that make tests/test_gpu_match.py meaningful, asserted without a device: every row of the form matrix
(tests/match_cases.py) plans the kernels it names -- cpk_batch_launch_plan, the launch plan for a device of 256 CUs that is
not there --, the rows together cover every sweep-family match-emitter entry of the kernel table, the oracle's lists alone
meet the caps the GPU suite puts on one-sided pairs, and the refresh-pass and gang shapes have the many segments per
region their suites describe."""
import pytest

import indel_cases as ic
import match_cases as mc
import test_gpu_gang as gang
import test_gpu_refresh_pass as rp

SETS = ("lds", "global", "queue", "dense-queue")


def _rows(which):
    if which == "lds":
        return [r.name for r in mc.LDS_ROWS]
    if which == "global":
        return [r.name for r in mc.GLOBAL_ROWS]
    return list(mc.QUEUE_ROWS if which == "queue" else mc.DENSE_QUEUE_ROWS)


def _global_width(mtype, monkeypatch):
    mc.set_row(monkeypatch, "GW1")
    return mc.first_global_width(mtype, mc.cpu_plan)


def _case_and_env(which, mtype, monkeypatch, threshold=0.01):
    if which == "lds":
        return mc.lds_case(mtype, threshold), {}
    if which == "global":
        # (at threshold 0 the pair at the edge alone: it emits every cell of its band, 0.5 and 1.2 million triples)
        return mc.global_case_at(mtype, _global_width(mtype, monkeypatch), threshold, second=threshold != 0), {}
    if which == "queue":
        return mc.queue_case(mtype, threshold), mc.QUEUE_ENV
    return mc.dense_queue_case(mtype, threshold), mc.DENSE_QUEUE_ENV


def _planned(which, row, mtype, monkeypatch):
    case, env = _case_and_env(which, mtype, monkeypatch)
    mc.set_row(monkeypatch, row, **env)
    return case, env, mc.cpu_plan(case)


ALL = [(which, row) for which in SETS for row in _rows(which)]


@pytest.mark.parametrize("mtype", mc.MTYPES)
@pytest.mark.parametrize("which,row", ALL)
def test_each_row_plans_the_expected_form(which, row, mtype, monkeypatch):
    """Family, mode, waves per SIMD, absolute positions and gang of both launches, 64 threads and the rows' memory, for every
    class of the batch; the class of the narrowest regions has room for every build, so there the row's kernels themselves
    are asked for, nothing demoted."""
    case, env, classes = _planned(which, row, mtype, monkeypatch)
    cap = int(env.get("CPECAN_MAX_WAVES_PER_CU", 0))
    assert classes and sum(c["regions"] for c in classes) == len(case.problems)
    for c in classes:
        want = mc.class_expectation(row, mtype, c, cap)
        assert mc.class_kernels(c) == want, (row, mtype, c)
        assert (c["packed"], c["family"], c["threads"], c["nStates"]) == (0, mc.FAMILY_SWEEP, 64, mc.states(mtype)), c
        assert c["globalRows"] == (1 if which == "global" else 0), c
        gangs = (c["gangWaves"], c["gangWavesTrace"])
        assert gangs == ((2, 2) if row == "G" else (0, 0)), c
    if which != "queue":  # (one wave per CU: no build for three puts a wave more on it, see match_cases.queue_case)
        assert mc.class_kernels(classes[0]) == mc.expected(row, mtype), (row, mtype, classes[0])
    if which in ("lds", "global") and mc.expected(row, mtype)[0].mode != mc.MODE_WHOLE:
        # (per class wherever the class holds no degenerate and no 33-diagonal region; over the batch in any case)
        wide = [c for c in classes if c["maxWidth"] > 100]
        assert wide and all(c["items"] >= 3 * c["regions"] for c in wide), classes
        assert sum(c["items"] for c in classes) >= 3 * len(case.problems), classes
    if which in ("queue", "dense-queue"):  # fewer waves than regions, than items: every wave takes a second one
        for c in classes:
            assert c["waves"] < c["regions"], c
            assert c["mode"] != mc.MODE_FORWARD or c["wavesTrace"] < c["items"], c


def test_lds_batch_has_a_class_per_width_group(monkeypatch):
    """Widths 9, 64, 65 (with the degenerate and the ragged problem) / 129 / 193 / 257: four wide classes."""
    mc.set_row(monkeypatch, "W1")
    for mtype in mc.MTYPES:
        classes = mc.cpu_plan(mc.lds_case(mtype, 0.01))
        assert [(c["regions"], c["maxWidth"]) for c in classes] == [(6, 100), (1, 129), (1, 193), (1, 257)], classes


def test_global_edge_is_found_by_stepping_the_planner(monkeypatch):
    """Found by stepping the planner, not written down: the last width with LDS rows and the first with global rows, and
    the interval they were seen in when the suite was written (689..692 cells of five states, 1077..1080 of three)."""
    for mtype, (lo, hi) in ((0, (689, 692)), (2, (1077, 1080))):
        w = _global_width(mtype, monkeypatch)
        assert lo <= w <= hi, (mtype, w)
        mc.set_row(monkeypatch, "GW1")
        assert not mc.cpu_plan(mc.global_case_at(mtype, w - 1, second=False))[-1]["globalRows"]
        assert all(c["globalRows"] for c in mc.cpu_plan(mc.global_case_at(mtype, w)))


def test_the_matrix_covers_the_kernel_table(monkeypatch):
    """Completeness guard: the sweep-family match-emitter variants of kKernelTable are exactly the kernels the matrix plans
    -- the first launch and the traceback launch of every row, both state counts, every class of the LDS, global and
    dense-queue batches.  A variant added to the table without a row fails here, and so does a row whose variant is gone.

    Out of this guard, run elsewhere: the packed kernels (cpk_packed.inl) by test_gpu_parity.py (test_packed_kernel_*, the
    split packed classes by test_packed_split_*) and test_gpu_indel.py / test_gpu_expect.py for their emitters; the team
    kernels (cpk_team.inl) by test_gpu_parity.py (test_team_*), test_gpu_indel.py and test_gpu_expect.py; the other emitters
    of the sweep family by test_gpu_forward.py, test_gpu_indel.py, test_gpu_expect.py and test_gpu_model_slots.py."""
    table = {(k["S"], k["mode"], k["fast"], k["wps"], k["abs"], k["gang"]) for k in mc.kernel_table()
             if k["family"] == mc.FAMILY_SWEEP and k["emit"] == mc.EMIT_MATCH}
    assert all(not (k["inSweep"] or k["slots"] or k["dynamic"] or k["width"]) for k in mc.kernel_table()
               if k["family"] == mc.FAMILY_SWEEP and k["emit"] == mc.EMIT_MATCH)
    planned = {}
    for which in ("lds", "global", "dense-queue"):
        for row in _rows(which):
            for mtype in mc.MTYPES:
                _, _, classes = _planned(which, row, mtype, monkeypatch)
                for c in classes:
                    for key in mc.form_keys(c):
                        planned.setdefault(key, "%s/%s/%d" % (which, row, mtype))
    missing, gone = table - set(planned), set(planned) - table
    assert not missing, "built variants (S, mode, fast, wps, abs, gang) that no row runs: %s" % sorted(missing)
    assert not gone, "rows whose variant is not in the table: %s" % {k: planned[k] for k in gone}


@pytest.mark.parametrize("mtype", mc.MTYPES)
@pytest.mark.parametrize("which", SETS)
def test_the_oracle_alone_meets_the_caps(which, mtype, monkeypatch):
    """Every non-degenerate problem emits pairs, and at threshold 0.01 the pairs within the gate's slack of the threshold
    are at most half of what the GPU suite lets stand on one side only."""
    for threshold in (mc.THRESHOLDS if which in ("lds", "global") else (0.01,)):
        case, _ = _case_and_env(which, mtype, monkeypatch, threshold)
        for (sx, sy, _, _, _), lst in zip(case.problems, mc.oracle_lists(case)):
            if not sx or not sy:
                assert len(lst) == 0
                continue
            assert len(lst) >= min(len(sx), len(sy)) // 4 >= 1, (case.name, len(sx), len(sy), len(lst))
            assert 2 * ic.near_threshold(lst, threshold) <= ic.one_sided_allowed(threshold, len(lst)) or threshold == 0, \
                (case.name, len(sx), len(lst), ic.near_threshold(lst, threshold))


# ---- the premise of test_gpu_refresh_pass.py and test_gpu_gang.py: many segments per region under the wide expansion ----
def _items_per_region(monkeypatch, mtype, problems, pkw):
    mc.set_row(monkeypatch, "A2")  # two launches, every region in a wide class: what both suites force
    problems = tuple(tuple(p) + (False, False) if len(p) == 3 else tuple(p) for p in problems)
    classes = mc.cpu_plan(mc.Case("premise", mtype, problems, pkw))
    assert sum(c["regions"] for c in classes) == len(problems)
    return classes


@pytest.mark.parametrize("mtype", mc.MTYPES)
def test_refresh_pass_regions_have_many_segments(mtype, monkeypatch):
    narrow, wide = rp.EXPANSIONS
    for w in rp.WIDTHS:
        sx, sy, a = rp._pair(w)
        (c,) = _items_per_region(monkeypatch, mtype, [(sx, sy, a)], rp._pkw(0.01, wide))
        assert c["items"] >= max(1, (len(sx) + len(sy)) // 50), (w, c["items"])
        (c,) = _items_per_region(monkeypatch, mtype, [(sx, sy, a)], rp._pkw(0.01, narrow))
        assert c["items"] == (1 if w <= 2 * narrow + 1 and len(sx) + len(sy) < 50 else 2), (w, c["items"])  # what the docstring says


@pytest.mark.parametrize("width,mtype", [(63, 0), (64, 2), (65, 0), (65, 2), (127, 0), (128, 2), (129, 0), (157, 0), (157, 2)])
def test_gang_width_regions_have_many_segments(width, mtype, monkeypatch):
    wide = gang.WIDTH_EXPANSIONS[1]
    for p in gang._width_problems(width):
        (c,) = _items_per_region(monkeypatch, mtype, [p], dict(threshold=0.01, diagonalExpansion=wide, **gang.SHORT))
        assert c["items"] >= (len(p[0]) + len(p[1])) // 50 >= 2, (width, c["items"])
