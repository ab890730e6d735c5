"""
Record what bluest_cov_project writes (X, f, gpmax, it, count, info) for the rows covproj_cases.bits_cases() of
tests/covproj_cases.py, as the library of the CURRENT checkout computes them on the GPU, into the .npz file named on the command
line:

    python tools/gen_golden_covproj_bits.py OUT.npz

tests/golden/covproj_bits_parent.npz was recorded this way from the commit before proj()'s eigensolver moved into
csrc/jacobi.hpp; tests/test_gpu_covproj_bits.py holds every later build to those bits.  The output path is mandatory and the tool
refuses to write into tests/golden: the committed record is not to be regenerated from newer code.  The inputs are seeded, the
file holds results only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import covproj_cases as cc
    import test_gpu_covproj_abi as abi
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_covproj_bits.py OUT.npz")
    out = os.path.abspath(sys.argv[1])
    if os.path.dirname(out) == os.path.join(ROOT, "tests", "golden"):
        sys.exit("refusing to write into tests/golden: the committed record stays the parent commit's")
    data = {}
    for row in cc.bits_cases():
        rec = cc.bits_record(abi.solo, row)
        data.update(rec)
        print("%-26s it=%d count=%d info=%d f=%r" % (row["name"], rec[row["name"] + "/it"], rec[row["name"] + "/count"],
                                                     rec[row["name"] + "/info"], float(rec[row["name"] + "/f"])))
    np.savez(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
