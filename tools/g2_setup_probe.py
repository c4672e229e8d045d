"""Times the G2 half of a setup against the G1 half on one device (profiles/g2_setup.md).

Every figure is a host clock around one blocking library call on host buffers: the call ends in a stream synchronisation and includes the download
of its result (288 B per G2 point, 144 B per G1 point).  Each shape is warmed once, then timed `--reps` times; minimum and median are printed.
The first call on a fresh handle is timed separately: it builds the handle's table of bls.GenG2.

    python tools/g2_setup_probe.py [--reps 7] [--sizes 4096,65536]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
S_TEST = 1927409816240961209460912649124


def fr_mont(k):
    v = (k % R) * ((1 << 256) % R) % R
    return np.array([[(v >> (64 * j)) & (2 ** 64 - 1) for j in range(4)]], dtype=np.uint64)


def timed(fn, reps):
    fn()                                                   # warm-up of this shape
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="4096,65536")
    args = ap.parse_args()
    import gokzg_amd as kz
    if kz.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing to measure")
    sizes = [int(s) for s in args.sizes.split(",")]
    sec = fr_mont(S_TEST)
    out = {}
    kz.FFTSettings(4).close()                              # runtime and code objects loaded before anything is timed
    fs = kz.FFTSettings(4)
    t0 = time.perf_counter()
    first = fs.generate_testing_setup_g2(sec, sizes[0])
    out["g2_first_call_fresh_handle_n%d_ms" % sizes[0]] = round((time.perf_counter() - t0) * 1e3, 3)
    assert fs.g2_table_builds() == 1
    t0 = time.perf_counter()
    again = fs.generate_testing_setup_g2(sec, sizes[0])
    out["g2_second_call_n%d_ms" % sizes[0]] = round((time.perf_counter() - t0) * 1e3, 3)
    assert np.array_equal(first, again)
    for n in sizes:
        out["g2_setup_n%d" % n] = timed(lambda: fs.generate_testing_setup_g2(sec, n), args.reps)
        out["g1_setup_n%d" % n] = timed(lambda: fs.generate_testing_setup_g1(sec, n), args.reps)
        g2, g1 = out["g2_setup_n%d" % n]["min_ms"], out["g1_setup_n%d" % n]["min_ms"]
        out["g2_share_of_full_setup_n%d" % n] = round(g2 / (g1 + g2), 3)
    n = sizes[-1]
    pts = fs.generate_testing_setup_g2(sec, n)
    out["g2_to_compressed_n%d" % n] = timed(lambda: fs.to_compressed_g2(pts), args.reps)
    assert fs.g2_table_builds() == 1
    fs.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
