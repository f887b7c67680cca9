"""CPU: every device-pointer entry point of include/mi355_msm.h has a test that pins its stream ordering.  The header is read as
text; stream_cases.COVERED names, per symbol, the test that runs the call with a late producer; the named test must exist in its
module, which is read as text too (nothing that needs a GPU is imported).  A new _device call cannot land without such a test."""
import os
import re

import stream_cases as st
from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    return set(re.findall(r"\b(mi355_msm_\w+_device|mi355_msm_run_async)\s*\(", text))


def test_every_device_pointer_call_is_covered():
    symbols = header_symbols()
    assert len(symbols) >= 21 and "mi355_msm_domain_scan_device" in symbols and "mi355_msm_run_async" in symbols
    covered = set(st.COVERED)
    assert symbols == covered, {"without a stream test": sorted(symbols - covered), "not in the header": sorted(covered - symbols)}


def test_every_named_test_exists():
    sources = {}
    for symbol, where in st.COVERED.items():
        module, _, test = where.partition("::")
        assert module and test, (symbol, where)
        if module not in sources:
            path = os.path.join(ROOT, "tests", module + ".py")
            assert os.path.exists(path), (symbol, where)
            sources[module] = open(path).read()
        assert re.search(r"^def %s\(" % re.escape(test), sources[module], flags=re.M), (symbol, where)
        assert "stream" in sources[module]
