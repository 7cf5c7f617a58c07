"""Run as a child process by tests/test_gpu_viterbi.py with CPECAN_LIB pointing at the exact-logAdd library
(`make -C cpecan_amd/csrc exact`).  Viterbi decoding has no logAdd: that build must give the same regions, states, ops and the
same bits of every logP as the model (tests/viterbi_model.py), like the default build.  All cases in one object, one run.
Prints one line per case and exits non-zero on the first difference."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from cpecan_amd import api, viterbi  # noqa: E402
import viterbi_cases as vc  # noqa: E402


def main():
    assert "exact" in os.path.basename(api.LIB_PATH), api.LIB_PATH
    for c in vc.cases():
        got = viterbi.viterbi_path(vc.model_pair(c.model)[0], c.sx, c.sy, vc.anchors_of(c), vc.lib_params(c), c.ragged_left,
                                   c.ragged_right)
        vc.assert_equals_model(c, got)
        print("exact: %s: logP %r, %d regions, %d ops" % (c.name, got.logP, len(got.regions), len(got.ops)), flush=True)
    print("exact: viterbi results equal", flush=True)


if __name__ == "__main__":
    main()
