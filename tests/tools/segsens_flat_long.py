#!/usr/bin/env python3
"""
`exact_sensitivities` with all prior weight on k = 0 at lengths of your choice (default: 2048, the library's limit, where the
solve kernel asks for 98 KB of dynamic LDS), against the softmax-weighted flat profiles of tests/gauss_sensitivity_oracle.py:
`check_flat_profiles` of tests/test_gpu_segment_sensitivity_tiles.py, which keeps T = 1376 in the suite.  Prints the deviations
and the wall times; an AssertionError above the bars (1e-10 on log_marginal and expected_logL, 1e-8 on grad and fisher).

    python tests/tools/segsens_flat_long.py [T ...]
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_gpu_segment_sensitivity_tiles import check_flat_profiles

for T in [int(v) for v in sys.argv[1:]] or [2048]:
    check_flat_profiles(T)
