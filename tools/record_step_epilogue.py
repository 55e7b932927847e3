"""Record what a library computes on the cases of tests/test_gpu_step_epilogue.py: the float32 parameters after 1 and 5 steps
of every case (tests/step_epilogue_cases.py), as one .npz.  Run on the commit whose results are the reference -- the parent
of a change that must not alter a bit -- twice, and keep the file only if both recordings are identical:

  python tools/record_step_epilogue.py a.npz && python tools/record_step_epilogue.py b.npz --same-as a.npz
  cp a.npz tests/golden/step_epilogue/parent.npz

Prints every case's launch count.  Needs the GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import step_epilogue_cases as SC  # noqa: E402
from tensor_ops_amd.hipt import HipT  # noqa: E402


def main():
    out = sys.argv[1]
    T = HipT(0)
    rec = {}
    for case in SC.CASES:
        got, launches = SC.run(T, case)
        print(case[0], "launches of a step:", launches, "(the test asserts %d)" % case[-1])
        for steps in SC.STEPS:
            for key, a in zip(SC.keys(case, steps), got[steps]):
                assert a.dtype == np.float32 and np.all(np.isfinite(a)), key
                rec[key] = a
    np.savez(out, **rec)
    print("recorded", len(rec), "arrays,", sum(a.nbytes for a in rec.values()), "bytes ->", out)
    if "--same-as" in sys.argv:
        with np.load(sys.argv[sys.argv.index("--same-as") + 1]) as other:
            assert sorted(other.files) == sorted(rec), "different cases"
            diff = [k for k in rec if not np.array_equal(other[k], rec[k])]
        assert not diff, "the two recordings differ: %s" % diff[:8]
        print("identical to", sys.argv[sys.argv.index("--same-as") + 1])


if __name__ == "__main__":
    main()
