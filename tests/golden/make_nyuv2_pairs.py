"""Writes tests/golden/nyuv2_pairs_parent.npz: what nyuv2.PairSource returned for tests/_mde_frames.py's frames BEFORE it learned
--include_location / --normalize / --include_originals (run once on that commit: python tests/golden/make_nyuv2_pairs.py).
Per case of _mde_frames.CASES, GOLDEN_BATCHES consecutive batches of GOLDEN_B pairs at seed GOLDEN_SEED, as float32."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _mde_frames as F  # noqa: E402

out = {}
for case in F.CASES:
    src = F.source(case)
    for b in range(F.GOLDEN_BATCHES):
        x, y = src.next_batch()
        out['%s/x%d' % (case, b)], out['%s/y%d' % (case, b)] = x.numpy(), y.numpy()
np.savez_compressed(os.path.join(HERE, 'nyuv2_pairs_parent.npz'), **out)
print({k: v.shape for k, v in out.items()})
