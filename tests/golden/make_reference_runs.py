#!/usr/bin/env python3
"""Writes tests/golden/reference_runs.json.gz: the cases of tests/reference_run_cases.py and what the reference itself
computed on them.  Run where the reference tree exists, after `make -C oracle ref` (the reference's two source files on
the stand-in headers of oracle/ref_standin/, with oracle/ref_driver.c as main).  DATA ONLY: inputs and recorded outputs.

  make_reference_runs.py                    write the case file, run oracle/_ref/cpecan_ref_driver, write the fixture
  make_reference_runs.py --driver PATH      another build of the driver (oracle/_ref/cpecan_ref_driver_asan)
  make_reference_runs.py --check            write nothing: fail unless the run gives the committed fixture byte for byte

For every thresholded case the reference also runs at threshold 0, and the case is refused if any score of those lists
lies within max(2, 2e-5 * threshold * 1e7) of threshold * 1e7 -- the slack parity.assert_pairs_match would grant a
one-sided pair: the case is then drawn again (another seed in reference_run_cases.py), not excused.
"""
import argparse
import gzip
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import reference_run_cases as rr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", default=os.path.join(ROOT, "oracle", "_ref", "cpecan_ref_driver"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        data = rr.fixture_bytes(args.driver, work)
    if args.check:
        if gzip.decompress(data) != gzip.decompress(open(rr.FIXTURE, "rb").read()):
            raise SystemExit("the run differs from %s" % rr.FIXTURE)
        print("the run gives %s" % os.path.basename(rr.FIXTURE))
        return
    with open(rr.FIXTURE, "wb") as f:
        f.write(data)
    print("wrote %s: %d cases, %d bytes" % (os.path.basename(rr.FIXTURE), len(rr.all_cases()), len(data)))


if __name__ == "__main__":
    main()
