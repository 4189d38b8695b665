"""Record tests/golden/corr_span_parent.npz: the fits of tests/test_gpu_corr_span.py's cases with
the knob left alone, by a library from before the knob existed.

    GPAR_HIP_LIB=/path/to/parent/libgparhip.so python tests/golden/make_corr_span_parent.py

(needs an MI355X; the parent is the commit before "corr_span" was added)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gpar-at-scale_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import test_gpu_corr_span as T  # noqa: E402

out = {}
for kind, s, m in T.CASES:
    fr = T.fit(T.batch(kind, s, m)[0], span=None)
    key = T.golden_key(kind, s, m)
    out[key + "_nlml"] = fr.nlml
    out[key + "_theta"] = fr.theta
    print(key, fr.nlml, flush=True)
np.savez(os.path.join(HERE, "corr_span_parent.npz"), **out)
