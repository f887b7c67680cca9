#!/usr/bin/env python3
"""Pull the scalar-field literals the reference holds -- modulus, multiplicative generator and (BLS12-377) the 2-adicity written in its
derivation note -- out of its sources into tests/golden/fr_constants.json (data, not code; run where the reference tree exists).

  ARKC bls12_377/src/fields/fr.rs:24-25   modulus, generator = 22;  :7  s = 47
  ARKC bls12_381/src/fields/fr.rs:4-5     modulus, generator = 7
"""
import json
import os
import re

ARKC = "/root/reference/open-division/prize4-msm-wasm/snarkify/zprize-prize4-15ac8c55-arkworks-curves"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out = {}
    for fam in ("bls12_377", "bls12_381"):
        src = open(os.path.join(ARKC, fam, "src", "fields", "fr.rs")).read()
        d = {"modulus": re.search(r"#\[modulus = \"(\d+)\"\]", src).group(1), "generator": re.search(r"#\[generator = \"(\d+)\"\]", src).group(1)}
        mm = re.search(r"^/// s = (\d+)$", src, flags=re.M)
        if mm:
            d["two_adicity"] = mm.group(1)
        out[fam] = d
    out["source"] = ("ARKC bls12_377/src/fields/fr.rs:24-25 (modulus, generator), :7 (s); bls12_381/src/fields/fr.rs:4-5; "
                     "decimal literals, normal form; extracted by tools/extract_fr_consts.py")
    with open(os.path.join(ROOT, "tests", "golden", "fr_constants.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
