"""Helper of tests/test_gpu_options.py (run in an interpreter of its own, because the scanline switches ADC_SO_FAST / ADC_SO_DPP are
read once per process): python tests/option_family_probe.py CASE...  Every named case (tests/cases.py) matches three times on one
handle -- the second Match on runs on the arm depth assumed from the first, which is what lets the last aggregation pass move
into the first scanline pass -- and every map is compared with the oracle's disp_final bit for bit.  Prints one JSON line:
{case: {"bad": [differing pixels per Match], "fused": counter 13, "seam_redos": counter 4, "segments": counter 5}}."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(names):
    import adcensus_amd as A
    from oracle import pyoracle
    from tests import cases
    orc = pyoracle.load("auto")
    out = {}
    for name in names:
        left, right, opt = cases.make_case(name)
        want = orc.run(left, right, opt, stages=["disp_final"])["disp_final"].view(np.uint32)
        st = A.ADCensusStereo(device=0)
        if not st.Initialize(left.shape[1], left.shape[0], cases.to_product_option(opt)):
            raise RuntimeError("%s: Initialize failed: %s" % (name, A.last_error()))
        try:
            bad = [int((st.match(left, right).view(np.uint32) != want).sum()) for _ in range(3)]
            out[name] = {"bad": bad, "fused": int(st.debug_counter(13)), "seam_redos": int(st.debug_counter(4)),
                         "segments": int(st.debug_counter(5))}
        finally:
            st.Release()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
