"""Run as a child process by tests/test_gpu_dense.py with CPECAN_LIB pointing at the diagnostic library
(`make -C cpecan_amd/csrc exact`: logAdd as the reference's operations one for one, impl/pairwiseAligner.c:287-307).
The comparisons of test_rows_match_the_oracle_trace at tolerance zero: every forward value of every state, F.match + B.match
of every emitted cell and every total used must EQUAL the oracle's.  Prints one line per case and exits non-zero on the
first difference."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from cpecan_amd import api, dense  # noqa: E402
import dense_cases as dc  # noqa: E402


def main():
    assert "exact" in os.path.basename(api.LIB_PATH), api.LIB_PATH
    for c in dc.cases():
        rows = dense.forward_backward(dc.model_pair(c.model)[0], c.sx, c.sy, dc.anchors_of(c), dc.lib_params(c), c.ragged_left,
                                      c.ragged_right)
        print("exact: " + dc.compare_with_oracle(c, rows, 0.0), flush=True)
    print("exact: dense rows equal", flush=True)


if __name__ == "__main__":
    main()
