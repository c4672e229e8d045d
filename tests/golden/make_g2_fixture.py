#!/usr/bin/env python3
"""Extracts the first 65 "setup_G2" entries of the reference's eth/trusted_setup.json into trusted_setup_g2.json (data only).

Run where a checkout of the reference exists (never on a test machine):
    python tests/golden/make_g2_fixture.py <path of the go-kzg checkout>
The fixture also pins the SHA-256 of the whole G2 array (the 4096 entries as concatenated 96-byte strings), the same pin
trusted_setup_sha256.json carries.  65 entries cover [s^n]G2 for every n <= 64 (CheckProofMulti) and [s]G2 (eth).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
COUNT = 65


def main():
    ref = sys.argv[1]
    ts = json.load(open(os.path.join(ref, "eth", "trusted_setup.json")))
    g2 = ts["setup_G2"]
    out = {"source": "eth/trusted_setup.json setup_G2[:%d]" % COUNT,
           "setup_G2_sha256": hashlib.sha256(b"".join(bytes.fromhex(h) for h in g2)).hexdigest(),
           "setup_G2": g2[:COUNT]}
    with open(os.path.join(HERE, "trusted_setup_g2.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
