"""
Record plan.phi and plan.eval (one and two candidates) of the plans of tests/step_bits_cases.py as the library of the CURRENT
checkout computes them on the GPU, into the .npz file named on the command line:

    python tools/gen_golden_step_bits.py OUT.npz

tests/golden/step_bits_parent.npz was recorded this way from the commit before the evaluation kernels' cross-lane reductions and
prologues were rewritten; tests/test_gpu_step_bits.py holds every later build to those bits.  The output path is mandatory and
the tool refuses to write into tests/golden: the committed record is not to be regenerated from newer code.  (To compare two
builds, record each into a file of its own and compare the arrays.)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import step_bits_cases as sbc
    from bluest_amd.plan import Plan
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_step_bits.py OUT.npz")
    out = os.path.abspath(sys.argv[1])
    if os.path.dirname(out) == os.path.join(ROOT, "tests", "golden"):
        sys.exit("refusing to write into tests/golden: the committed record stays the parent commit's")
    data = {}
    for name in sbc.NAMES:
        n, Lg, outs, m1, M2, expect, regular = sbc.problem(name)
        if not regular:
            os.environ["BLUEST_NO_REGULAR_FOLD"] = "1"
        else:
            os.environ.pop("BLUEST_NO_REGULAR_FOLD", None)
        plan = Plan(n, Lg, outs, max_candidates=2)
        cfg = plan.launch_config(1)
        for k, want in expect.items():
            assert cfg[k] == want, (name, k, cfg)
        rec = sbc.record(plan, name, m1, M2)
        data.update(rec)
        print("%-10s regular=%d cfg=%s st1=%s st2=%s" % (name, regular, {k: cfg[k] for k in expect}, rec[name + "/st1"].ravel(), rec[name + "/st2"].ravel()))
    np.savez(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
