"""csrc/dev.hpp is the one seam between the product and the simulator build (DESIGN: "The product / simulator seam"): no other
source of the library calls the HIP runtime, launches a kernel itself or names the runtime's stream and event types."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bulletproofs-r1cs-gadgets_amd", "csrc")
FILES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip", ".inc")) and f != "dev.hpp")


def test_there_are_sources_to_look_at():
    assert len(FILES) >= 20 and "msm_run.hpp" in FILES and "api_prove.hpp" in FILES


@pytest.mark.parametrize("fn", FILES)
def test_only_dev_hpp_touches_the_hip_runtime(fn):
    with open(os.path.join(CSRC, fn)) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    for pat in (r"\bhip[A-Z]\w*\s*\(", r"hipLaunchKernelGGL", r"HIPCHK", r"\bhipStream_t\b", r"\bhipEvent_t\b"):
        hits = [text.count("\n", 0, m.start()) + 1 for m in re.finditer(pat, text)]
        assert not hits, "csrc/%s, line(s) %s: %s belongs in dev.hpp (dev_stream_t, dev_event_t, launch_kernel and the dev_* functions)" % (fn, hits, pat)
