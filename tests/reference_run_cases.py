"""The small constructed inputs the reference itself is run on (oracle/Makefile target `ref`, oracle/ref_driver.c), and the
committed record of what it computed (tests/golden/reference_runs.json.gz, written by tests/golden/make_reference_runs.py).
tests/test_reference_runs_cpu.py holds the oracle to the records, tests/test_gpu_reference_runs.py the HIP library.

Device-free: the library is not loaded here.  Where a case of consumer_cases, indel_cases or the GPU files' generators
already has the right shape its inputs are used.  Every sequence is at most 300 bases.

A case is a dict:
  name, ops        ops: the reference functions the driver calls on it, of
                   pairs indels forward expect shifted_mea      (model + sequences + anchors + params + ragged)
                   mea reweight shift scores overlap            (explicit lists)
  model            a key of MODELS
  params           threshold, minDiagsBetweenTraceBack, traceBackDiagonals, diagonalExpansion, splitMatrixBiggerThanThis,
                   dynamicAnchorExpansion, gapGamma (the float of the parameter block: MEA)
  ragged           (left, right)
  sx, sy, anchors  str, str, [(x, y, expansion)]
  pairs, gx, gy    [(weight, x, y)]; lX, lY; gamma (the double of reweightAlignedPairs2)
"""
import functools
import gzip
import io
import json
import os
import random
import subprocess
import zlib

import numpy as np

import consumer_cases as cc
import reference_cases as rc

PROB_1 = 10000000
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_runs.json.gz")
DP_OPS = ("pairs", "indels", "forward", "expect", "shifted_mea")
LIST_KEYS = {"pairs": ("match",), "indels": ("imatch", "gapx", "gapy")}
RAGGED = ((False, False), (True, False), (False, True), (True, True))
F085 = cc.F085
_ALPHABET = "AaCcGgTt" * 11 + "N"  # test_gpu_parity._ALPHABET: both cases, a little N

FIVE_STATE, FIVE_STATE_ASYM, THREE_STATE, THREE_STATE_ASYM = 0, 1, 2, 3


# ---- models ----
def _normalised(T, E, S):
    """hmm_normalise in its own order of operations (a running sum from the left, then one division per entry)."""
    T, E = list(T), list(E)
    for frm in range(S):
        total = 0.0
        for to in range(S):
            total += T[frm * S + to]
        for to in range(S):
            T[frm * S + to] = T[frm * S + to] / total
    for s in range(S):
        total = 0.0
        for k in range(16):
            total += E[s * 16 + k]
        for k in range(16):
            E[s * 16 + k] = E[s * 16 + k] / total
    return T, E


@functools.lru_cache(maxsize=None)
def models():
    """name -> dict(type[, T, E]).  The two symmetric defaults carry no numbers; "trained" is the reference's own trained
    five-state-asymmetric HMM (tests/golden/trained_hmm_cPecanEmTest.txt); "threeStateAsymmetric" is the randomised,
    normalised HMM of test_gpu_forward._model_pair (the same generator and seed)."""
    mtype, T, _, E = rc.trained_hmm_numbers()
    assert mtype == FIVE_STATE_ASYM
    rng = random.Random(51 + THREE_STATE_ASYM)
    T3 = [0.05 + rng.random() for _ in range(9)]
    E3 = [0.05 + rng.random() for _ in range(48)]
    T3, E3 = _normalised(T3, E3, 3)
    return {"fiveState": dict(type=FIVE_STATE), "threeState": dict(type=THREE_STATE),
            "trained": dict(type=FIVE_STATE_ASYM, T=T, E=E), "threeStateAsymmetric": dict(type=THREE_STATE_ASYM, T=T3, E=E3)}


MODEL_NAMES = ("fiveState", "threeState", "trained", "threeStateAsymmetric")


def states(model):
    return 5 if models()[model]["type"] in (FIVE_STATE, FIVE_STATE_ASYM) else 3


# ---- sequences ----
def _rand_seq(rng, n, alphabet=_ALPHABET):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _related(rng, n, m=None, sub=0.15, alphabet=_ALPHABET):
    """n bases, and a copy with substitutions cut or padded to m bases; from 20 bases on the copy has lost three bases a
    third of the way along and gained three others at two thirds: both gap lists get something to hold."""
    m = n if m is None else m
    sx = _rand_seq(rng, n, alphabet)
    sy = "".join(rng.choice(alphabet) if rng.random() < sub else ch for ch in sx)
    if n >= 20:
        sy = sy[:n // 3] + sy[n // 3 + 3:2 * n // 3] + _rand_seq(rng, 3, alphabet) + sy[2 * n // 3:]
    return sx, (sy + _rand_seq(rng, max(0, m - n), alphabet))[:m]


def _with_indels(rng, n, deletions, insertions, block):
    """(sx of n bases, sy, the true pairs): sy is sx without `deletions` runs of `block` bases, with `insertions` runs of
    `block` other bases and with 5 % substitutions."""
    sx = _rand_seq(rng, n)
    starts = rng.sample(range(20, n - 20, 2 * block + 10), deletions + insertions)
    gone = {i for s in starts[:deletions] for i in range(s, s + block)}
    sy, true = [], []
    for i, ch in enumerate(sx):
        if i in starts[deletions:]:
            sy += list(_rand_seq(rng, block))
        if i not in gone:
            true.append((i, len(sy)))
            sy.append(rng.choice(_ALPHABET) if rng.random() < 0.05 else ch)
    return sx, "".join(sy), true


def _params(threshold=0.01, minDiags=1000, traceBack=40, expansion=20, split=3000 * 3000, dynamic=0, gapGamma=0.5):
    return dict(threshold=threshold, minDiagsBetweenTraceBack=minDiags, traceBackDiagonals=traceBack,
                diagonalExpansion=expansion, splitMatrixBiggerThanThis=split, dynamicAnchorExpansion=dynamic,
                gapGamma=float(np.float32(gapGamma)))


def _dp(name, ops, model, sx, sy, anchors=(), ragged=(False, False), **pkw):
    return dict(name=name, ops=list(ops), model=model, params=_params(**pkw), ragged=tuple(bool(r) for r in ragged),
                sx=sx, sy=sy, anchors=[tuple(int(v) for v in a) for a in anchors])


def _lists(name, ops, pairs=(), gx=(), gy=(), lX=None, lY=None, sx="", sy="", gamma=0.0, gapGamma=0.5):
    return dict(name=name, ops=list(ops), model="fiveState", params=_params(gapGamma=gapGamma), ragged=(False, False),
                sx=sx, sy=sy, anchors=[], pairs=[tuple(int(v) for v in p) for p in pairs],
                gx=[tuple(int(v) for v in p) for p in gx], gy=[tuple(int(v) for v in p) for p in gy],
                lX=len(sx) if lX is None else lX, lY=len(sy) if lY is None else lY, gamma=float(gamma))


# The generator of each group of cases.  A group whose lists hold a score within threshold_margin of its threshold is drawn
# again -- tests/golden/make_reference_runs.py refuses it -- by raising its number here.
DRAW = {"wide65-threeStateAsymmetric": 1, "banded150": 1}


def _drawn(group):
    return random.Random(9100 + zlib.crc32(group.encode()) % 1000 + 1000 * DRAW.get(group, 0))


ALL_DP = ("pairs", "indels", "forward", "expect")
NUMBERS = ("forward", "expect")

# the unbanded pair whose three lists at threshold 0 hold every cell of their domain
CLOSED_FORM = "ragged40x30-fiveState-0-0"


def closed_form_lengths(lX, lY):
    """Threshold 0, no band, no ragged end: a match at every (x, y); a gap in X at every x in front of, between and
    behind the bases of Y, and the other way round."""
    return lX * lY, lX * (lY + 1), (lX + 1) * lY


@functools.lru_cache(maxsize=None)
def dp_cases():
    out = []
    # 1. the smallest shapes, every model, every function, threshold 0
    tiny = [("1x1", "A", "A"), ("1x5", "G", "AGTTC"), ("5x1", "CTGAC", "T"), ("AGCG", "AGCG", "AGTTCG")]
    for model in MODEL_NAMES:
        for tag, sx, sy in tiny:
            out.append(_dp("tiny-%s-%s" % (tag, model), ALL_DP, model, sx, sy, threshold=0.0))
    # 2. unanchored, the widest diagonal just under, at and over one group of 64 cells, and over two
    for k, (cells, model, threshold) in enumerate(((63, "threeStateAsymmetric", 0.0), (64, "fiveState", 0.01), (65, "trained", 0.2),
                                                   (129, "threeState", 0.01), (64, "trained", 0.01), (65, "threeStateAsymmetric", 0.01))):
        n = cells - 1
        sx, sy = _related(_drawn("wide%d-%s" % (cells, model)), n)
        ops = ALL_DP if threshold > 0 else ("pairs", "forward", "expect")
        out.append(_dp("wide%d-%s-%g" % (cells, model, threshold), ops, model, sx, sy, threshold=threshold))
    # 3. 300 x 280 under anchors of expansion 10 and a short traceback schedule: several tracebacks and refresh points
    sx, sy, true = _with_indels(_drawn("banded300x280"), 300, 6, 2, 5)
    assert (len(sx), len(sy)) == (300, 280)
    anchors = [(x, y, 10) for x, y in true[12::25]]
    for model, threshold in (("fiveState", 0.01), ("trained", 0.2), ("threeStateAsymmetric", 0.01)):
        out.append(_dp("banded300x280-%s-%g" % (model, threshold), ALL_DP, model, sx, sy, anchors, threshold=threshold,
                       minDiags=50, traceBack=7, expansion=10))
    # 4. cut by a small splitMatrixBiggerThanThis: two anchors 90 apart, matrices over 400 cells are split
    sx, sy, true = _with_indels(_drawn("split"), 130, 2, 1, 4)
    anchors = [(x, y, 8) for x, y in (true[10], true[104])]
    for model, ragged in (("fiveState", (False, False)), ("threeState", (True, True))):
        out.append(_dp("split-%s-%d-%d" % ((model,) + ragged), ALL_DP, model, sx, sy, anchors, ragged, threshold=0.01, expansion=8, split=400))
    # 5. the four ragged combinations of one 40 x 30 pair: threshold 0 under the default five-state model (every cell of
    #    every list), the numbers under every model
    sx, sy = _related(_drawn("ragged40x30"), 40, 30)
    for model in MODEL_NAMES:
        for rl, rr in RAGGED:
            ops = ALL_DP if model == "fiveState" else ("pairs",) + NUMBERS
            out.append(_dp("ragged40x30-%s-%d-%d" % (model, rl, rr), ops, model, sx, sy, (), (rl, rr), threshold=0.0))
    # 6. N-rich and lower case
    sx, sy = _related(_drawn("n-rich"), 70, 66, alphabet="ACGTNNNN")
    out.append(_dp("n-rich", ALL_DP, "fiveState", sx, sy, threshold=0.01))
    out.append(_dp("n-rich-asym", ALL_DP, "threeStateAsymmetric", sx, sy, ragged=(True, False), threshold=0.01))
    sx, sy = _related(_drawn("lower-case"), 66, 70, alphabet="acgt")
    out.append(_dp("lower-case", ALL_DP, "trained", sx, sy, threshold=0.01))
    out.append(_dp("lower-case-zero", ("indels", "forward"), "threeState", sx[:25], sy[:22], threshold=0.0))
    # 7. every model on one banded pair at the default threshold and at 0.2, ragged ends going round
    sx, sy, true = _with_indels(_drawn("banded150"), 150, 2, 2, 3)
    anchors = [(x, y, 10) for x, y in true[7::20]]
    for k, model in enumerate(MODEL_NAMES):
        for threshold in (0.01, 0.2):
            out.append(_dp("banded150-%s-%g" % (model, threshold), ALL_DP, model, sx, sy, anchors, RAGGED[(k + (threshold > 0.1)) % 4],
                           threshold=threshold, expansion=10))
    # 8. getShiftedMEAAlignment end to end on three pairs
    sx, sy, true = _with_indels(_drawn("shifted-mea-banded"), 120, 1, 1, 6)
    out.append(_dp("shifted-mea-banded", ("indels", "shifted_mea"), "fiveState", sx, sy, [(x, y, 12) for x, y in true[9::30]], threshold=0.01,
                   expansion=12, gapGamma=0.5))
    sx, sy = _related(_drawn("shifted-mea-unanchored"), 63, 60)
    out.append(_dp("shifted-mea-unanchored", ("indels", "shifted_mea"), "threeStateAsymmetric", sx, sy, threshold=0.01, gapGamma=F085))
    sx, sy = "CAAAAAAAAAGTTGCATTTCCG", "CAAAAAAGTTGCATTTTTTCCG"  # gaps inside homopolymers: the shift has somewhere to go
    out.append(_dp("shifted-mea-homopolymer", ("indels", "shifted_mea"), "trained", sx, sy, threshold=0.01, gapGamma=0.0))
    return tuple(out)


MEA_NAMES = ("tie_record_rounding", "tie_64_apart", "tie_start_score", "length_1", "length_63", "length_64", "length_65",
             "empty_list_with_gaps", "empty_chain", "one_by_one", "gamma_zero", "no_gap_lists", "walk_64_pair", "walk_65_pair",
             "walk_65_sentinel", "runoff_64_65_66", "handoff_lane_0", "handoff_lane_63")
REWEIGHT_NAMES = ("n_0", "n_255", "n_256", "n_257", "floor_at_zero", "mass_at_bound")


@functools.lru_cache(maxsize=None)
def consumer_cases():
    out = []
    mea = cc.mea_cases()
    for name in MEA_NAMES:
        c = mea[name]
        out.append(_lists("mea-" + name, ("mea",), c["pairs"], c["gx"], c["gy"], c["lX"], c["lY"], gapGamma=c["gamma"]))
    # n = 0 without gap lists, and n = 64 under gamma 0
    out.append(_lists("mea-n0-bare", ("mea",), (), (), (), 3, 2))
    c = mea["length_64"]
    out.append(_lists("mea-length_64-gamma0", ("mea",), c["pairs"], c["gx"], c["gy"], c["lX"], c["lY"], gapGamma=0.0))
    rw = cc.reweight_cases()
    for name in REWEIGHT_NAMES:
        c = rw[name]
        gammas = c["gammas"] if name in ("floor_at_zero", "n_257") else (0.5, 0.0) if name in ("n_0", "mass_at_bound") else (F085, 50.0)
        for g in gammas:
            tag = "f085" if g == F085 else "%g" % g
            out.append(_lists("reweight-%s-%s" % (name, tag), ("reweight",), c["pairs"], lX=c["lX"], lY=c["lY"], gamma=g))
    for name, c in cc.shift_cases().items():
        out.append(_lists("shift-" + name, ("shift",), c["pairs"], sx=c["sx"], sy=c["sy"]))
    c = cc.IDENTITY
    out.append(_lists("scores-identity", ("scores",), c["pairs"], sx=c["sx"], sy=c["sy"]))
    rng = random.Random(9200)
    sx, sy = _related(rng, 33, 41)
    pairs = [(rng.randrange(1, PROB_1 + 1), i, i + rng.randrange(0, 8)) for i in range(33)]
    out.append(_lists("scores-random", ("scores",), pairs, sx=sx, sy=sy))
    out.append(_lists("scores-one-pair", ("scores",), [(3333333, 0, 2)], sx="a", sy="CNA"))
    out.append(_lists("scores-empty-sequences-listed", ("scores",), [(PROB_1, 0, 0), (1, 1, 1), (7, 2, 2)], sx="NNN", sy="nnn"))
    # filterToRemoveOverlap: (x, y, expansion) sorted by x then y; overlaps in x (one row twice), in y (one column twice)
    # and in both (a pair that goes backwards in y)
    overlap = [(0, 0, 3), (1, 1, 3), (1, 2, 3), (2, 3, 4), (3, 3, 4), (4, 5, 4), (5, 4, 5), (6, 6, 5), (7, 7, 5), (7, 9, 6),
               (8, 7, 6), (9, 10, 6), (10, 11, 7)]
    out.append(_lists("overlap-x-y-both", ("overlap",), overlap))
    out.append(_lists("overlap-none", ("overlap",), [(i, 2 * i, 1) for i in range(6)]))
    out.append(_lists("overlap-empty", ("overlap",), []))
    return tuple(out)


def all_cases():
    out = dp_cases() + consumer_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def threshold_margin(threshold):
    """The slack parity.assert_pairs_match grants a one-sided pair near the threshold; no recorded score lies inside it
    (tests/golden/make_reference_runs.py refuses the case), so no comparison with a record needs the excuse."""
    return max(2.0, 2e-5 * threshold * PROB_1)


# ---- the case file of oracle/ref_driver.c, its records, and the fixture made of both ----
def _flat(rows):
    return " ".join(str(int(v)) for r in rows for v in r)


def case_file_text(cases):
    lines = []
    for c in cases:
        m, p = models()[c["model"]], c["params"]
        lines.append("case %s %s" % (c["name"], ",".join(c["ops"])))
        if "T" in m:
            lines.append("hmm %d %s" % (m["type"], " ".join(repr(float(v)) for v in list(m["T"]) + list(m["E"]))))
        else:
            lines.append("model %d" % m["type"])
        lines.append("params %r %d %d %d %d %d %r" % (p["threshold"], p["minDiagsBetweenTraceBack"], p["traceBackDiagonals"],
                                                       p["diagonalExpansion"], p["splitMatrixBiggerThanThis"],
                                                       p["dynamicAnchorExpansion"], p["gapGamma"]))
        lines.append("ragged %d %d" % c["ragged"])
        lines.append("sx =" + c["sx"])
        lines.append("sy =" + c["sy"])
        lines.append("anchors %d %s" % (len(c["anchors"]), _flat(c["anchors"])))
        if "pairs" in c:
            lines.append("lens %d %d" % (c["lX"], c["lY"]))
            for key in ("pairs", "gx", "gy"):
                lines.append("%s %d %s" % (key, len(c[key]), _flat(c[key])))
            lines.append("gamma %r" % c["gamma"])
        lines.append("end")
    return "\n".join(lines) + "\n"


def parse_records(text):
    """{case name: {key: flat integer list | hex string | list of hex strings}} from the driver's output."""
    out, cur = {}, None
    for line in text.splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "case":
            cur = out.setdefault(tok[1], {})
            assert not cur, "case %s recorded twice" % tok[1]
        elif tok[0] == "end":
            cur = None
        elif tok[0] == "list":
            assert len(tok) == 3 + 3 * int(tok[2])
            cur[tok[1]] = [int(v) for v in tok[3:]]
        elif tok[0] == "ints":
            assert len(tok) == 3 + int(tok[2])
            cur[tok[1]] = [int(v) for v in tok[3:]]
        elif tok[0] == "double":
            cur[tok[1]] = tok[2]
        elif tok[0] == "doubles":
            assert len(tok) == 3 + int(tok[2])
            cur[tok[1]] = tok[3:]
        else:
            raise ValueError("unknown record line: %s" % line[:80])
    return out


def shadow_of(case):
    """The same case at threshold 0, lists only: what make_reference_runs.py looks at for scores near the threshold."""
    ops = [op for op in case["ops"] if op in LIST_KEYS]
    if not ops or case["params"]["threshold"] <= 0:
        return None
    return dict(case, name="shadow:" + case["name"], ops=ops, params=dict(case["params"], threshold=0.0))


def near_threshold(case, shadow_record):
    """The scores of the threshold-0 lists that lie within threshold_margin of the case's threshold."""
    t = case["params"]["threshold"]
    edge, margin = t * PROB_1, threshold_margin(t)
    found = []
    for key, flat in shadow_record.items():
        s = triples(flat)[:, 0]
        found += [(key, int(v)) for v in s[np.abs(s - edge) <= margin]]
    return found


def run_driver(driver, cases, workdir):
    path = os.path.join(workdir, "reference_runs.cases")
    with open(path, "w") as f:
        f.write(case_file_text(cases))
    return parse_records(subprocess.run([driver, path], check=True, stdout=subprocess.PIPE).stdout.decode())


def fixture_bytes(driver, workdir):
    """Runs every case (and the threshold-0 shadow of every thresholded one) through the driver and returns the bytes of
    tests/golden/reference_runs.json.gz: the same input gives the same bytes (mtime 0, keys sorted)."""
    cases = list(all_cases())
    shadows = [s for s in map(shadow_of, cases) if s]
    records = run_driver(driver, cases + shadows, workdir)
    refused = ["%s: %r" % (c["name"], near_threshold(c, records["shadow:" + c["name"]])) for c in cases
               if shadow_of(c) and near_threshold(c, records["shadow:" + c["name"]])]
    if refused:
        raise SystemExit("scores within the margin of the threshold, draw these again (DRAW):\n  " + "\n  ".join(refused))
    doc = dict(models=models(), cases=[dict(c, out=records[c["name"]]) for c in cases])
    raw = json.dumps(doc, sort_keys=True, separators=(",", ":")).encode()
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", fileobj=buf, mode="wb", compresslevel=9, mtime=0) as f:
        f.write(raw)
    return buf.getvalue()


# ---- the committed records ----
@functools.lru_cache(maxsize=None)
def fixture():
    """{"models": ..., "cases": [case with "out": {key: value}]}: lists as flat integer lists, doubles as hex strings."""
    with gzip.open(FIXTURE, "rb") as f:
        return json.loads(f.read().decode())


def hexes(values):
    return [float.fromhex(v) for v in values]


def triples(flat):
    return np.asarray(flat, dtype=np.int64).reshape(-1, 3)
