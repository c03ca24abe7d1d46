"""Two `bench.py --dump-outputs` directories array for array: same files, shapes, types and bytes.
usage: compare_dumps.py DIR_A DIR_B   (exit status 1 on any difference)"""
import glob
import os
import sys

import numpy as np

a, b = sys.argv[1], sys.argv[2]
fa = sorted(os.path.basename(f) for f in glob.glob(a + "/*.npy"))
fb = sorted(os.path.basename(f) for f in glob.glob(b + "/*.npy"))
print("files", fa == fb, len(fa))
ok = fa == fb and len(fa) > 0
for f in fa if fa == fb else []:
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    print(f, x.shape, x.dtype, "EQUAL" if same else "DIFFERS")
    ok = ok and same
print("ALL EQUAL" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
