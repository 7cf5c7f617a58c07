"""ctypes mirror of include/cpecan_em.h: pair-HMM training by expectation maximisation (cPecanEm.py).

`train(...)` is the whole of cPecanEm: sample the alignments, upload them once, iterate E-steps on the resident batches
and M-steps on the host, write the model file.  `Trainer` exposes the same with the sequences added one by one.
"""
import ctypes as C

from . import api
from . import realign

# Every symbol include/cpecan_em.h declares.
EXPORTS = [
    "cpecan_em_options_default", "cpecan_hmm_equalise", "cpecan_hmm_set_jukes_cantor", "cpecan_hmm_tie_emissions",
    "cpecan_hmm_randomise", "cpecan_em_random", "cpecan_em_sample", "cpecan_em_blast_matrix",
    "cpecan_em_write_lastz_matrix", "cpecan_em_fasta_gc", "cpecan_em_write_model", "cpecan_em_trainer_create",
    "cpecan_em_trainer_destroy", "cpecan_em_trainer_read_fasta", "cpecan_em_trainer_add_sequence",
    "cpecan_em_trainer_set_devices", "cpecan_em_train", "cpecan_em_trainer_timing",
    "cpecan_em_trainer_set_concurrent_trials", "cpecan_em_trainer_alignments", "cpecan_em_trainer_set_viterbi_training",
]

MODEL_TYPES = {"fiveState": api.fiveState, "fiveStateAsymmetric": api.fiveStateAsymmetric,
               "threeState": api.threeState, "threeStateAsymmetric": api.threeStateAsymmetric}


class EmOptions(C.Structure):
    """cpecan_em_options: cPecanEm.py's options with its defaults (cpecan_em_options_default)."""
    _fields_ = [("modelType", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32), ("randomStart", C.c_int32),
                ("useDefaultModelAsStart", C.c_int32), ("trainEmissions", C.c_int32), ("tieEmissions", C.c_int32),
                ("outputTrialHmms", C.c_int32), ("setJukesCantorStartingEmissions", C.c_double),
                ("maxAlignmentLengthPerJob", C.c_int64), ("maxAlignmentLengthToSample", C.c_int64),
                ("seed", C.c_uint64), ("inputModel", C.c_char_p), ("blastScoringMatrixFile", C.c_char_p),
                ("updateTheBand", C.c_int32)]


class EmTiming(C.Structure):
    _fields_ = [("setupMs", C.c_double), ("iterationsMs", C.c_double), ("iterations", C.c_int64),
                ("cigars", C.c_int64), ("jobs", C.c_int64), ("realignMs", C.c_double), ("replanMs", C.c_double),
                ("handoffMs", C.c_double)]


_bound = False


def _lib():
    global _bound
    L = realign._lib()
    if not _bound:
        vp, hp = C.c_void_p, C.POINTER(api.Hmm)
        i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        L.cpecan_em_options_default.argtypes = [C.POINTER(EmOptions)]
        L.cpecan_em_options_default.restype = None
        L.cpecan_hmm_equalise.argtypes = [hp]
        L.cpecan_hmm_set_jukes_cantor.argtypes = [hp, C.c_double]
        L.cpecan_hmm_tie_emissions.argtypes = [hp]
        L.cpecan_hmm_randomise.argtypes = [hp, C.POINTER(C.c_uint64)]
        L.cpecan_em_random.argtypes = [C.POINTER(C.c_uint64)]
        L.cpecan_em_random.restype = C.c_double
        L.cpecan_em_sample.argtypes = [C.POINTER(realign._Cigar), C.c_int64, C.c_int64, C.c_int64, C.c_uint64, i64p, i64p,
                                       i64p, dp]
        L.cpecan_em_blast_matrix.argtypes = [hp, C.c_double, dp, dp, dp]
        L.cpecan_em_write_lastz_matrix.argtypes = [C.c_char_p, dp, C.c_double, C.c_double]
        L.cpecan_em_fasta_gc.argtypes = [C.c_char_p, i64p, i64p]
        L.cpecan_em_fasta_gc.restype = C.c_int64
        L.cpecan_em_write_model.argtypes = [hp, dp, C.c_int, C.c_char_p]
        L.cpecan_em_trainer_create.argtypes = [C.POINTER(vp), C.POINTER(EmOptions), C.POINTER(realign.RealignOptions),
                                               C.c_int]
        L.cpecan_em_trainer_destroy.argtypes = [vp]
        L.cpecan_em_trainer_destroy.restype = None
        L.cpecan_em_trainer_read_fasta.argtypes = [vp, C.c_char_p]
        L.cpecan_em_trainer_read_fasta.restype = C.c_int64
        L.cpecan_em_trainer_add_sequence.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int64]
        L.cpecan_em_trainer_set_devices.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
        L.cpecan_em_trainer_set_concurrent_trials.argtypes = [vp, C.c_int]
        L.cpecan_em_trainer_set_viterbi_training.argtypes = [vp, C.c_int, C.c_double]
        L.cpecan_em_train.argtypes = [vp, C.POINTER(realign._Cigar), C.c_int64, C.c_char_p, hp, dp]
        L.cpecan_em_trainer_timing.argtypes = [vp, C.POINTER(EmTiming)]
        L.cpecan_em_trainer_alignments.argtypes = [vp, C.POINTER(i64p), C.POINTER(i64p), i64p]
        _bound = True
    return L


def _b(s):
    return s.encode() if isinstance(s, str) else s


def em_options(**overrides):
    """cpecan_em_options with cPecanEm's defaults; modelType may be given by name ("threeState")."""
    o = EmOptions()
    _lib().cpecan_em_options_default(C.byref(o))
    for k, v in overrides.items():
        if k == "modelType" and isinstance(v, str):
            v = MODEL_TYPES[v]
        if k in ("inputModel", "blastScoringMatrixFile") and v is not None:
            v = _b(v)
        if k == "setJukesCantorStartingEmissions" and v is None:
            v = -1.0
        setattr(o, k, v)
    return o


def em_realign_options(diagonalExpansion=10, splitMatrixBiggerThanThis=3000, **overrides):
    """The realign options cPecanEm passes by default ("--diagonalExpansion=10 --splitMatrixBiggerThanThis=3000"), with
    splitMatrixBiggerThanThis as the side of the square, as on the command line; other overrides as realign_options."""
    ro = realign.realign_options(diagonalExpansion=diagonalExpansion, **overrides)
    ro.params.splitMatrixBiggerThanThis = int(splitMatrixBiggerThanThis) ** 2
    return ro


# ---- model operations of cPecanEm.py's Hmm ----
def hmm_equalise(h):
    api._check(_lib().cpecan_hmm_equalise(C.byref(h)), "cpecan_hmm_equalise")
    return h


def hmm_set_jukes_cantor(h, divergence):
    api._check(_lib().cpecan_hmm_set_jukes_cantor(C.byref(h), float(divergence)), "cpecan_hmm_set_jukes_cantor")
    return h


def hmm_tie_emissions(h):
    api._check(_lib().cpecan_hmm_tie_emissions(C.byref(h)), "cpecan_hmm_tie_emissions")
    return h


def hmm_randomise(h, seed):
    s = C.c_uint64(seed)
    api._check(_lib().cpecan_hmm_randomise(C.byref(h), C.byref(s)), "cpecan_hmm_randomise")
    return h


def sample(cigars, max_per_job, max_to_sample, seed):
    """cpecan_em_sample: (indices of the sampled cigars, number of jobs, sampled alignment length)."""
    cigars = list(cigars)
    arr, keep = _pack(cigars)
    order = (C.c_int64 * max(1, len(cigars)))()
    n, jobs, length = C.c_int64(), C.c_int64(), C.c_double()
    api._check(_lib().cpecan_em_sample(arr, len(cigars), int(max_per_job), int(max_to_sample), int(seed), order,
                                       C.byref(n), C.byref(jobs), C.byref(length)), "cpecan_em_sample")
    return list(order[:n.value]), jobs.value, length.value


def blast_matrix(h, gc_fraction):
    """makeBlastScoringMatrix: (16 match scores, gap open, gap extend), unrounded."""
    scores = (C.c_double * 16)()
    go, ge = C.c_double(), C.c_double()
    api._check(_lib().cpecan_em_blast_matrix(C.byref(h), float(gc_fraction), scores, C.byref(go), C.byref(ge)),
               "cpecan_em_blast_matrix")
    return list(scores), go.value, ge.value


def write_lastz_matrix(path, scores, gap_open, gap_extend):
    arr = (C.c_double * 16)(*scores)
    api._check(_lib().cpecan_em_write_lastz_matrix(_b(path), arr, float(gap_open), float(gap_extend)),
               "cpecan_em_write_lastz_matrix")


def write_model(h, path, running=()):
    running = list(running)
    arr = (C.c_double * max(1, len(running)))(*running)
    api._check(_lib().cpecan_em_write_model(C.byref(h), arr, len(running), _b(path)), "cpecan_em_write_model")


def _pack(cigars):
    arr = (realign._Cigar * max(1, len(cigars)))()
    keep = []
    for i, c in enumerate(cigars):
        arr[i] = c._to_c(keep)
    return arr, keep


class Trainer:
    """cpecan_em_trainer: sequences in, cigars in, a trained model file out."""

    def __init__(self, options=None, realign_options=None, device=0):
        self._h = C.c_void_p()
        self.options = options or em_options()
        self.realign_options = realign_options or em_realign_options()
        api._check(_lib().cpecan_em_trainer_create(C.byref(self._h), C.byref(self.options),
                                                   C.byref(self.realign_options), device), "cpecan_em_trainer_create")

    def close(self):
        if self._h:
            _lib().cpecan_em_trainer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def read_fasta(self, path):
        return api._check(_lib().cpecan_em_trainer_read_fasta(self._h, _b(path)), "cpecan_em_trainer_read_fasta")

    def add_sequence(self, header, seq):
        seq = _b(seq)
        api._check(_lib().cpecan_em_trainer_add_sequence(self._h, _b(header), seq, len(seq)),
                   "cpecan_em_trainer_add_sequence")

    def set_devices(self, devices):
        devices = list(devices)
        arr = (C.c_int * max(1, len(devices)))(*devices)
        api._check(_lib().cpecan_em_trainer_set_devices(self._h, arr, len(devices)), "cpecan_em_trainer_set_devices")

    def set_concurrent_trials(self, n):
        """Random-restart trials per kernel launch (1 to 8; 1: one after another); more trials run in rounds."""
        api._check(_lib().cpecan_em_trainer_set_concurrent_trials(self._h, int(n)), "cpecan_em_trainer_set_concurrent_trials")

    def set_viterbi_training(self, on=True, pseudo_count=1.0):
        """Viterbi training (hard EM): the E-step counts along the most probable path of every sampled alignment, on top of
        pseudo_count in every bin.  Not with updateTheBand, several concurrent trials or several devices."""
        api._check(_lib().cpecan_em_trainer_set_viterbi_training(self._h, int(bool(on)), float(pseudo_count)),
                   "cpecan_em_trainer_set_viterbi_training")

    def train(self, cigars, output_model):
        """Runs every trial; returns (best Hmm, its running likelihoods)."""
        cigars = [c if isinstance(c, realign.Cigar) else realign.Cigar.parse(c) for c in cigars]
        arr, keep = _pack(cigars)
        best = api.Hmm()
        n_iter = max(1, self.options.iterations)
        running = (C.c_double * n_iter)()
        api._check(_lib().cpecan_em_train(self._h, arr, len(cigars), _b(output_model), C.byref(best), running),
                   "cpecan_em_train")
        return best, list(running[:self.options.iterations])

    def alignments(self):
        """cpecan_em_trainer_alignments: per sampled cigar the anchor runs (x, y, length, expansion) the last E-step of the
        last trial of an updateTheBand training ran on, as int64 arrays of shape (k, 4)."""
        import numpy as np
        runs, counts, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_int64()
        api._check(_lib().cpecan_em_trainer_alignments(self._h, C.byref(runs), C.byref(counts), C.byref(n)),
                   "cpecan_em_trainer_alignments")
        out, at = [], 0
        for i in range(n.value):
            k = counts[i]
            out.append(np.array(runs[4 * at:4 * (at + k)], dtype=np.int64).reshape(k, 4))
            at += k
        return out

    def timing(self):
        t = EmTiming()
        api._check(_lib().cpecan_em_trainer_timing(self._h, C.byref(t)), "cpecan_em_trainer_timing")
        return t


def train(sequence_files, cigars, output_model, device=0, devices=None, realign_options=None, **options):
    """cPecanEm in one call: sequence_files (fasta paths), cigars (Cigar objects or cigar lines), output_model (path);
    options are cpecan_em_options fields by name.  Returns (best Hmm, running likelihoods)."""
    with Trainer(em_options(**options), realign_options, device) as t:
        if devices:
            t.set_devices(devices)
        for path in sequence_files:
            t.read_fasta(path)
        return t.train(cigars, output_model)
