"""The count kernels of cpk_viterbi.inl and the resident form of a Viterbi object (cpecan_viterbi_run_counts, DESIGN.md section
13) on the GPU against the numpy definition, tests/viterbi_counts_model.py, on the cases of tests/viterbi_counts_cases.py: every
bin integer for integer, every logP bit for bit; every case alone under its own model, all cases in one object under budgets
that cut the run into launches, under both kernel forms, across model swaps, beside a plain run on the same object, and on the
exact-logAdd library in one child process."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import viterbi_cases as vc
import viterbi_counts_cases as cc
import viterbi_counts_model as cm
import viterbi_model as vm
from cpecan_amd import api, viterbi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXACT = os.path.join(ROOT, "cpecan_amd", "libcpecan_hip_exact.so")


def _same_bytes(a, b, what):
    assert a.transitions.tobytes() == b.transitions.tobytes() and a.emissions.tobytes() == b.emissions.tobytes(), what
    assert (a.nSteps, a.nNoPath) == (b.nSteps, b.nNoPath) and np.float64(a.logP).tobytes() == np.float64(b.logP).tobytes(), what


def _add(v, c):
    return v.add(c.sx, c.sy, vc.anchors_of(c), c.ragged_left, c.ragged_right)


_alone_cache = {}


def _alone(c, form=viterbi.FORM_AUTO):
    """The case alone under its own model and parameters: (Counts of the object, Counts of its one problem, launch forms)."""
    with viterbi.Viterbi(vc.model_pair(c.model)[0], vc.lib_params(c)) as v:
        v.set_form(form)
        v.set_keep_problem_counts(True)
        _add(v, c)
        total = v.run_counts()
        return total, v.problem_counts(0), v.launch_forms()


def _result(c):
    if c.name not in _alone_cache:
        _alone_cache[c.name] = _alone(c)
    return _alone_cache[c.name]


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_case_counts_equal_the_model_beside_a_plain_run(name):
    """1 and 4: the case under its own model.  Counts and logP equal the model; a plain run on the same object afterwards still
    equals viterbi_model; run_counts after that gives the counts again; the results of either are dropped by the other."""
    c = cc.case(name)
    want = cc.problem_counts(c)
    with viterbi.Viterbi(vc.model_pair(c.model)[0], vc.lib_params(c)) as v:
        v.set_keep_problem_counts(True)
        _add(v, c)
        total = v.run_counts()
        print("%s: %d steps, %d emissions, nNoPath %d, logP %r, count %r ms" % (name, total.nSteps, int(total.emissions.sum()), total.nNoPath,
                                                                                 total.logP, v.count_ms()))
        cm.assert_equal(total, want, name)
        cm.assert_equal(v.problem_counts(0), want, name)
        assert v.launch_forms().launches == 1
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            v.result(0)  # the ops stayed on the device
        v.run()
        vc.assert_equals_model(c, v.result(0))
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            v.problem_counts(0)
        again = v.run_counts()
        _same_bytes(again, total, name)
        _same_bytes(v.problem_counts(0), total, name)
    _same_bytes(_result(c)[0], total, name)


@functools.lru_cache(maxsize=None)
def _config_model(config):
    """Every case under the model and parameters of `config`: per case the [Counts] of its regions.  Computed once."""
    cfg = cc.case(config)
    om, p = vc.model_pair(cfg.model)[1], vc.oracle_params(cfg)
    out = []
    for c in cc.cases():
        m = vm.viterbi(om, c.sx, c.sy, vc.anchors_of(c), p, c.ragged_left, c.ragged_right)
        out.append(tuple(cm.regions(om.S, m, _region_inputs(c, p))))
    return tuple(out)


def _region_inputs(c, p):
    return [(bytes(c.sx)[x1:x2], bytes(c.sy)[y1:y2], rl, rr)
            for x1, y1, x2, y2, _, rl, rr in vm.regions_of(vc.anchors_of(c), len(c.sx), len(c.sy), p, c.ragged_left, c.ragged_right)]


@pytest.mark.parametrize("config", ("r_three", "p_no_path"))
def test_one_object_equals_the_model_under_every_budget(config):
    """1: every case in one object with keep_problem_counts on (an object holds one model and one set of parameters: those of
    `config`).  Per-problem counts and totals equal the model; logP is the sum over the contributing regions in region order.
    Under the default budget, a third of the whole and exactly the largest region's bytes every number is the same and the
    number of launches is not."""
    cfg = cc.case(config)
    S = cc.n_states(cfg)
    per_case = _config_model(config)
    want_total = cm.total(S, [r for regs in per_case for r in regs])
    assert want_total.nNoPath >= (1 if config == "p_no_path" else 0) and want_total.nSteps > 3000
    with viterbi.Viterbi(vc.model_pair(cfg.model)[0], vc.lib_params(cfg)) as v:
        v.set_keep_problem_counts(True)
        for i, c in enumerate(cc.cases()):
            assert _add(v, c) == i
        whole = sum(v.info(i)["deviceBytes"] for i in range(v.n))
        n_regions = sum(v.info(i)["nRegions"] for i in range(v.n))
        assert n_regions == sum(len(regs) for regs in per_case)
        largest = 1  # the largest single region's bytes: the refusals (host only) name them one after the other
        while True:
            v.set_budget(largest)
            try:
                v.resident_bytes()
                break
            except api.CpecanError as e:
                m = re.search(r"\(-4\).*needs (\d+) bytes", str(e))
                assert m and int(m.group(1)) > largest, str(e)
                largest = int(m.group(1))
        launches = []
        for budget in (viterbi.MAX_BYTES, max(largest, whole // 3), largest):
            v.set_budget(budget)
            inputs, scratch = v.resident_bytes()
            total = v.run_counts()
            f = v.launch_forms()
            print("%s: budget %d of %d bytes: %r, resident %d + %d bytes, logP %r, nNoPath %d" % (config, budget, whole, f, inputs, scratch,
                                                                                                    total.logP, total.nNoPath))
            assert f.lds + f.global_ == n_regions and inputs + scratch <= whole + 4 * (S * S + S * 16) * n_regions
            launches.append(f.launches)
            cm.assert_equal(total, want_total, (config, budget))
            for i, c in enumerate(cc.cases()):
                cm.assert_equal(v.problem_counts(i), cm.total(S, per_case[i]), (config, budget, c.name))
        assert launches[0] == 1 and 3 <= launches[1] < launches[2], launches


@pytest.mark.parametrize("form", viterbi.FORMS)
def test_every_kernel_form_gives_the_same_bytes(form):
    """2: the form forced on the small cases."""
    for name in cc.SMALL_CASE_NAMES:
        c = cc.case(name)
        total, problem, forms = _alone(c, form)
        n = forms.lds + forms.global_
        assert forms == ((1, n, 0) if form == viterbi.FORM_LDS else (1, 0, n)), (name, forms)
        _same_bytes(total, _result(c)[0], (name, form))
        _same_bytes(problem, _result(c)[1], (name, form))


def _all_counts(v):
    return [v.run_counts()] + [v.problem_counts(i) for i in range(v.n)]


# the default models of a type and its asymmetric twin hold the same numbers: that swap changes no answer, the other two do
@pytest.mark.parametrize("a,b,differ", (("fiveState", "fiveStateAsym", False), ("fiveStateAsym", "fiveStateNoLongOpen", True),
                                        ("threeState", "threeStateAsym", False), ("threeStateAsym", "threeStateNoEndY", True)))
def test_model_swap_keeps_the_inputs_and_changes_the_answer(a, b, differ):
    """3: run under A, set_model(B), run, set_model(A), run: the first and third results are the same bytes and the second is
    that of a fresh object created with B.  Models of one state count; another count is refused and changes nothing."""
    sa, sb = vc.model_pair(a)[0], vc.model_pair(b)[0]
    p = vc.lib_params(cc.case("r_three"))
    small = [cc.case(n) for n in cc.SMALL_CASE_NAMES]

    def fresh(sm):
        v = viterbi.Viterbi(sm, p)
        v.set_keep_problem_counts(True)
        for c in small:
            _add(v, c)
        return v

    with fresh(sa) as v, fresh(sb) as w:
        first = _all_counts(v)
        v.set_model(sb)
        with pytest.raises(api.CpecanError, match=r"\(-5\)"):
            v.problem_counts(0)  # results of the earlier run are dropped
        second = _all_counts(v)
        other = vc.model_pair("threeState" if a.startswith("five") else "fiveState")[0]
        with pytest.raises(api.CpecanError, match=r"\(-1\)"):
            v.set_model(other)
        v.set_model(sa)
        third = _all_counts(v)
        want = _all_counts(w)
    assert len(first) == len(small) + 1
    for i, (x, y, z, u) in enumerate(zip(first, second, third, want)):
        _same_bytes(x, z, (a, b, i))
        _same_bytes(y, u, (a, b, i))
    seen = first[0].transitions.tobytes() != second[0].transitions.tobytes() or first[0].logP != second[0].logP
    assert seen == differ, "a swap between models that differ must change the answer, one between equal models must not"


def test_exact_build_gives_the_same_bytes(tmp_path):
    """5: one child process on the exact-logAdd library, held to the bytes this process got."""
    assert os.path.exists(EXACT), "%s is missing: __graft_entry__.build() makes it (`make -C cpecan_amd/csrc exact`)" % EXACT
    arrays = {}
    for c in cc.cases():
        t = _result(c)[0]
        arrays[c.name + ".t"], arrays[c.name + ".e"] = t.transitions, t.emissions
        arrays[c.name + ".s"] = np.array([t.nSteps, t.nNoPath], dtype=np.int64)
        arrays[c.name + ".p"] = np.array([t.logP], dtype=np.float64)
    path = str(tmp_path / "counts.npz")
    np.savez(path, **arrays)
    env = dict(os.environ, CPECAN_LIB=EXACT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "viterbi_counts_exact_check.py"), path], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "viterbi counts equal" in r.stdout
