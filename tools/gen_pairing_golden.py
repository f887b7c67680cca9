#!/usr/bin/env python3
"""Write tests/golden/pairing/{bls12_377,bls12_381}.bin from the big-integer model of tests/pairing_cases.py: about two dozen pairs a
family -- both generators, random multiples a G1, b G2 with full-width a and b, -P, P or Q or both at infinity, flagged infinities with
junk coordinates -- each with its G1 and G2 image and the expected Gt image in both forms (Montgomery and canonical).  The GPU tests
read the files so that they never run the model; tests/test_pairing_model.py regenerates them byte for byte.
Run:  python tools/gen_pairing_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pairing_cases as pc  # noqa: E402

if __name__ == "__main__":
    os.makedirs(pc.GOLDEN, exist_ok=True)
    for F in pc.FAMILIES.values():
        raw = pc.golden_bytes(F)
        with open(pc.golden_path(F), "wb") as f:
            f.write(raw)
        print(pc.golden_path(F), len(raw), "bytes")
