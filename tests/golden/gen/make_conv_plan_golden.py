"""Records tests/golden/conv_plan_sweep.npz: every host-only answer of the fp32 conv planner (synthsr_conv3d_plan, the packed sizes of
synthsr_conv3d_pack_ex, the two weight-gradient routing queries) over the grid tests/test_conv_variants_cpu.py names in SWEEP_*.

    python tests/golden/gen/make_conv_plan_golden.py

Run it at the commit whose routing is to be pinned, or against a library built from that commit (SYNTHSR_HIP_LIB selects the
library that synthsr_amd loads).  No device is needed.  The sweep itself is test_conv_variants_cpu.plan_sweep, so the fixture and
the test that replays it cannot drift apart.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import test_conv_variants_cpu as t   # noqa: E402
from synthsr_amd import _lib         # noqa: E402

if __name__ == '__main__':
    table = t.plan_sweep(_lib.load())
    np.savez_compressed(t.GOLDEN_SWEEP, table=table, shapes=np.asarray(t.SWEEP_SHAPES, dtype=np.int64),
                        cin=np.asarray(t.SWEEP_CIN, dtype=np.int64), cout=np.asarray(t.SWEEP_COUT, dtype=np.int64),
                        kinds=np.asarray(t.SWEEP_KINDS, dtype=np.int64), arith=np.asarray(t.SWEEP_ARITH, dtype=np.int64),
                        columns=np.asarray(t.SWEEP_COLUMNS))
    print(t.GOLDEN_SWEEP, table.shape, os.path.getsize(t.GOLDEN_SWEEP), 'bytes; library', _lib.LIB_PATH)
