"""The error of the readout's canonical exponential over EVERY float32 in [-87, 0] (include/ext/mmf_hg_readout.h).

    python scripts/readout_exp_sweep.py [--jobs N]

cexp (tests/readout_restate.py holds the numpy form, the header the definition) is compared with float64 exp on all 1 118 699 521
bit patterns from -0.0 (0x80000000) to -87.0 (0xC2AE0000), in ulps of the correctly rounded float32 result.  Chunked numpy on the
CPU, no GPU; a few minutes on 8 processes.  The maximum, rounded up to the next half ulp, is CEXP_ULPS of tests/readout_restate.py.
Also reported: whether every result is a normal number, cexp(-0.0), and whether the results of ADJACENT float32 ever go the wrong way
(they do: an approximation with an error above half an ulp cannot promise otherwise; on a sample spaced wider than a few ulps of t the
function is monotone, which is what tests/test_readout_cpu.py checks)."""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import readout_restate as rr      # noqa: E402

FIRST, LAST = 0x80000000, 0xC2AE0000
STEP = 1 << 22


def piece(lo):
    hi = min(lo + STEP, LAST + 1)
    t = np.arange(lo, hi + 1 if hi <= LAST else hi, dtype=np.uint32).view(np.float32)      # one value of overlap: monotone across pieces
    got = rr.cexp(t)
    want = np.exp(t.astype(np.float64))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want) / ulp
    k = int(np.argmax(err))
    normal = bool((got >= np.finfo(np.float32).tiny).all())
    monotone = bool((got[1:] <= got[:-1]).all())                                           # bits ascending: t descending
    return float(err[k]), float(t[k]), normal, monotone


def main():
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(8, os.cpu_count() or 1)
    worst, at, normal, monotone = 0.0, 0.0, True, True
    with ProcessPoolExecutor(max_workers=jobs) as ex:
        for e, t, n, m in ex.map(piece, range(FIRST, LAST + 1, STEP)):
            if e > worst:
                worst, at = e, t
            normal, monotone = normal and n, monotone and m
    one = float(rr.cexp(np.float32(-0.0)))
    print(f"values {LAST - FIRST + 1}  max error {worst:.4f} ulp at t = {at!r}  all normal {normal}  monotone {monotone}  cexp(-0) = {one!r}")
    print(f"CEXP_ULPS = {np.ceil(worst * 2) / 2:.1f}  (tests/readout_restate.py has {rr.CEXP_ULPS})")


if __name__ == "__main__":
    main()
