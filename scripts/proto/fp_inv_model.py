"""Runner of the integer model of the lockstep modular inversion (csrc/fp_inv.cuh).  The model itself lives in tests/fp29_model.py (inv29: the kernel's
arithmetic limb for limb, with its invariants and bounds asserted) and the operands in tests/fp29_cases.py; tests/test_fp29_model.py runs both in the
suite.  This script prints what they find: python scripts/proto/fp_inv_model.py"""
import collections
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))

import fp29_cases as Cs          # noqa: E402
import fp29_model as F           # noqa: E402


def main():
    ic = Cs.inversion_cases()
    xs = list(dict.fromkeys(x for cl in ic.values() for x in cl if x))
    hist = collections.Counter(Cs._run(x)[1] for x in xs)
    worst = max(xs, key=lambda x: Cs._run(x)[2])
    found, runs = Cs.inversion_search()
    print("ok: %d operands; iterations until a = 0: %s" % (len(xs), sorted(hist.items())))
    print("needs all %d iterations: %d operands; wrong after %d: %d" % (F.FP_INV_ITERS, len(ic["needs_all_27"]), F.FP_INV_ITERS - 1, len(ic["wrong_after_26"])))
    print("search: %d runs of %d iterations, %d more full-length operands, longest %d" % (runs, Cs.SEARCH_ITERS, len(found), max(s for _, s in found)))
    print("max |u|, |v| = %.3f p at X = %s" % (Cs._run(worst)[2] / F.P, hex(worst)))


if __name__ == "__main__":
    main()
