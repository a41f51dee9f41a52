"""Op sequences beyond the 32 that tests/test_op_sequences.py pins (GPU box): the same op kinds on other grids of the list and with
other cameras, images, rays and fields.  python tools/extra_op_sequences.py [FIRST_VARIANT [END_VARIANT]]
A failed comparison is printed and the sweep goes on; any other error ends it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle as orc
orc.build()
import tests.test_op_sequences as t
from tests import op_sequences as S

lo = int(sys.argv[1]) if len(sys.argv) > 1 else 1
hi = int(sys.argv[2]) if len(sys.argv) > 2 else lo + 20
fails = 0
for variant in range(lo, hi):
    for seed in S.SEEDS:
        try:
            t.drive(orc, seed, variant=variant)
        except AssertionError as e:
            if e.__cause__ is not None and not isinstance(e.__cause__, AssertionError):
                print("ERR variant %d seed %d\n%s" % (variant, seed, e))
                sys.exit(3)
            fails += 1
            print("FAIL variant %d seed %d\n%s" % (variant, seed, e))
    S.sequence.cache_clear()
print("extra op sequences done: variants %d .. %d, failures: %d; comparisons by weight storage %s, ray casts %s"
      % (lo, hi - 1, fails, dict(sorted(t._SEEN["modes"].items())), t._SEEN["casts"]))
