#!/usr/bin/env python3
"""Records golden/lobpcg_bits.npz ON THE DEVICE, with the build in the tree.  Run from the repository root:

    python tests/golden/make_lobpcg_bits.py [FILE]

The cases, their inputs and the launches are those of tests/test_gpu_lobpcg_kernels.py (bits_cases): the int64 patterns of G and H of
the Gram step and of res2 and both ends of every column of W of the residual step, in all three mass forms.  Record it with the build
whose bits are to be kept, BEFORE a change to the kernels; the test then holds every later build to them.

Checked here, on the CPU: no stored SUM (G, H, res2; an entry of W is one fma and one product, and where 3, 7 or 5 divides the hashed
numerator its input is a 12-bit number itself) is a small dyadic number (a multiple of 2^-12, as every output of the exact cases of
lobpcg_cases.py is), whose sum need not have rounded.  The inputs are 12-bit numbers over 3, 7 and 5, so a sum of n products is near
N / (9 * 2^22) with an integer N, and where 9 (21, 15) divides N the rounding errors of the terms may cancel and leave that multiple
of 2^-22 itself -- a few entries in a hundred do, having rounded at every term all the same.  More than one in eight would mean
inputs that do not round, and is refused.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ehyb_spmv_gpu_amd as E  # noqa: E402
import test_gpu_lobpcg_kernels as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.BITS_FILE
    if E.device_count() < 1:
        raise SystemExit("no HIP device visible: the bits are the device's")
    bits = dict(T.bits_cases(E, E.DeviceBuffer(T.SCRATCH_DOUBLES)))
    short = 0
    for key, b in bits.items():
        v = b.view(np.float64)
        assert np.isfinite(v).all(), key
        if key.endswith("_W"):
            continue
        assert (v * 2.0 ** 12 != np.rint(v * 2.0 ** 12)).all(), f"{key}: a small dyadic value"
        short += int((v * 2.0 ** 30 == np.rint(v * 2.0 ** 30)).sum())
    total = sum(b.size for b in bits.values())
    sums = sum(b.size for key, b in bits.items() if not key.endswith("_W"))
    assert 8 * short <= sums, f"{short} of {sums} sums are multiples of 2^-30: the inputs do not round"
    np.savez_compressed(out, **bits)
    print(f"wrote {out}: {len(bits)} arrays, {total} values ({short} of {sums} sums multiples of 2^-30), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
