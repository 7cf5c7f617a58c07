"""Run as a child process by tests/test_gpu_viterbi_counts.py with CPECAN_LIB pointing at the exact-logAdd library
(`make -C cpecan_amd/csrc exact`) and the path of an .npz that holds what the default build counted.  Decoding and counting
have no logAdd: this build must give the same bytes.  Every case alone under its own model.  Prints one line per case and
exits non-zero on the first difference."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from cpecan_amd import api, viterbi  # noqa: E402
import viterbi_cases as vc  # noqa: E402
import viterbi_counts_cases as cc  # noqa: E402


def main():
    assert "exact" in os.path.basename(api.LIB_PATH), api.LIB_PATH
    want = np.load(sys.argv[1])
    for c in cc.cases():
        with viterbi.Viterbi(vc.model_pair(c.model)[0], vc.lib_params(c)) as v:
            v.add(c.sx, c.sy, vc.anchors_of(c), c.ragged_left, c.ragged_right)
            got = v.run_counts()
        assert got.transitions.tobytes() == want[c.name + ".t"].tobytes() and got.emissions.tobytes() == want[c.name + ".e"].tobytes(), c.name
        assert [got.nSteps, got.nNoPath] == want[c.name + ".s"].tolist(), c.name
        assert np.float64(got.logP).tobytes() == want[c.name + ".p"].tobytes(), (c.name, got.logP)
        print("exact: %s: %d steps, logP %r" % (c.name, got.nSteps, got.logP), flush=True)
    print("exact: viterbi counts equal", flush=True)


if __name__ == "__main__":
    main()
