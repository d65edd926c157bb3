"""The depth models' shared kernel helpers and whole-frame sweep against the commit before they were shared:
tests/golden/depth_parent_digests.npz was written on that commit by `python tools/regression_digest.py --depth` (the tool,
copied into that checkout, uses only what both trees have).  Per named output -- the entry points of tdg_cgan*.hip on seeded
inputs, and infer_full / evaluate / metrics of paper_cgan and sample_full of paper_sampler -- the SHA-256 of the raw bytes
must be the same: the consolidation moved no bit."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_paper_cgan import DEV

pytestmark = pytest.mark.gpu


def test_depth_outputs_equal_the_parent_commit():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import regression_digest as RD
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'depth_parent_digests.npz'))
    want = {str(n): (str(h), float(s)) for n, h, s in zip(gold['names'], gold['sha256'], gold['sums'])}
    got = RD.depth_digests(DEV)
    assert sorted(got) == sorted(want)
    assert sum(k.startswith('kernel/') for k in got) == 71 and sum(k.startswith('model/') for k in got) == 15
    wrong = ['%s: sum %r, was %r' % (k, got[k][1], want[k][1]) for k in sorted(want) if got[k][0] != want[k][0]]
    assert not wrong, 'outputs differ from the parent commit:\n' + '\n'.join(wrong)
