#!/usr/bin/env python3
"""Write tests/golden/compressed/<curve>.json: 64 arkworks compressed records per curve with the uncompressed record and the status
each must decode to, valid and invalid kinds mixed.  Everything comes from the Python model (tests/codec_cases.py, oracle/pymodel.py);
the host test and the GPU test of the point codec both read the files.
Run:  python tools/gen_compressed_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codec_cases as kc  # noqa: E402
import pymodel as pm  # noqa: E402


def main():
    out_dir = os.path.join(ROOT, "tests", "golden", "compressed")
    os.makedirs(out_dir, exist_ok=True)
    for name in kc.CURVE_NAMES:
        curve = pm.CURVES[name]
        recs = kc.fixture_records(name)
        statuses, unc = kc.expected(curve, b"".join(recs), serialized=True)
        rb = 2 * curve.coord_bytes
        doc = {"curve": name, "record_bytes": curve.coord_bytes,
               "note": "compressed: x little-endian, bit 6 of the last byte infinity, bit 7 y is the larger root; status 0 decoded, 1 malformed, 2 no point",
               "records": [r.hex() for r in recs], "status": statuses,
               "uncompressed": [unc[i * rb:(i + 1) * rb].hex() for i in range(len(recs))]}
        assert len(recs) == 64 and min(statuses) == 0 and {1, 2} <= set(statuses)
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")
        print(name, {s: statuses.count(s) for s in sorted(set(statuses))})


if __name__ == "__main__":
    main()
