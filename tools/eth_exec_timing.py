#!/usr/bin/env python3
"""Wall times of the batched execution-layer calls (EthSettings.point_evaluation_precompile_batch, kzg_to_versioned_hash_batch,
verify_kzg_commitments_against_transactions_batch) on the n = 4096 setup.  profiles/eth_exec.md records a run.

  precompile   8 / 64 / 512 / 4096 / 65 536 valid rows against verify_kzg_proof_batch on the same rows split into their fields, in the same
               process: the call the library had before, which the new one follows with one SHA-256 block per lane more.  Five repeats of
               each; the spread of a call is max - min of its repeats.
  hashes       1 k / 64 k / 1 M commitments against a hashlib loop on one host thread.
  tx check     64 / 4096 blocks of four blobs each (one blob transaction per block), the flattening of the Python lists excluded.

Prints one JSON line per measurement.  Nothing is asserted: whether the precompile at 4096 rows lies within the run-to-run spread of the
older call is reported as `within_spread`.

    eth_exec_timing.py [--rows 8,64,512,4096,65536] [--hashes 1000,65536,1048576] [--blocks 64,4096] [--reps 5]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gokzg_amd as kz  # noqa: E402
import eth_exec_cases as ec  # noqa: E402
import verify_images as vi  # noqa: E402
from oracle import koracle as ko  # noqa: E402

S = 1337          # the secret of tests/golden/trusted_setup_g2.json
DISTINCT = 16     # distinct valid rows; larger batches repeat them (a lane's work does not depend on its neighbours)


def times(f, reps):
    f()
    out = []
    for _ in range(reps):
        t = time.perf_counter(); f(); out.append((time.perf_counter() - t) * 1e3)
    return out


def stats(ts):
    return {"min": round(min(ts), 3), "median": round(float(np.median(ts)), 3), "max": round(max(ts), 3), "spread": round(max(ts) - min(ts), 3)}


def valid_rows(rng):
    """(commitment, z, y, proof) byte rows that verify on the fixture setup: C = [y + (s - z) t] G1, pi = [t] G1"""
    rows = []
    for _ in range(DISTINCT):
        t, z, y = (rng.randrange(1, ko.R_MOD) for _ in range(3))
        rows.append((bytes(vi.compress_scalar(y + (S - z) * t)), z.to_bytes(32, "little"), y.to_bytes(32, "little"), bytes(vi.compress_scalar(t))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8,64,512,4096,65536")
    ap.add_argument("--hashes", default="1000,65536,1048576")
    ap.add_argument("--blocks", default="64,4096")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs, lag)
    eth.set_setup_g2(fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"][:2]), dtype=np.uint8)))
    rng = random.Random(1)

    rows = valid_rows(rng)
    for count in ints(a.rows):
        pick = [rows[i % DISTINCT] for i in range(count)]
        inputs = np.frombuffer(b"".join(ec.versioned_hash(c) + z + y + c + pi for c, z, y, pi in pick), dtype=np.uint8).reshape(count, 192)
        c48, zs, ys, pi48 = (np.frombuffer(b"".join(r[k] for r in pick), dtype=np.uint8).reshape(count, -1) for k in range(4))
        assert eth.point_evaluation_precompile_batch(inputs).min() == 1 and eth.verify_kzg_proof_batch(c48, zs, ys, pi48).min() == 1
        new = times(lambda: eth.point_evaluation_precompile_batch(inputs), a.reps)
        old = times(lambda: eth.verify_kzg_proof_batch(c48, zs, ys, pi48), a.reps)
        new2 = times(lambda: eth.point_evaluation_precompile_batch(inputs), a.reps)      # the new call once more, after the old one
        sn, so = stats(new), stats(old)
        print(json.dumps({"what": "precompile", "rows": count, "precompile_ms": sn, "verify_kzg_proof_ms": so, "precompile_again_ms": stats(new2),
                          "median_difference_ms": round(sn["median"] - so["median"], 3),
                          "within_spread": bool(sn["median"] - so["median"] <= max(sn["spread"], so["spread"]))}), flush=True)

    for count in ints(a.hashes):
        comm = np.frombuffer(rng.randbytes(48 * count), dtype=np.uint8).reshape(count, 48)
        dev = times(lambda: eth.kzg_to_versioned_hash_batch(comm), a.reps)
        raw = comm.tobytes()
        t = time.perf_counter()
        want = b"".join(b"\x01" + hashlib.sha256(raw[48 * i:48 * i + 48]).digest()[1:] for i in range(count))
        host_ms = (time.perf_counter() - t) * 1e3
        assert eth.kzg_to_versioned_hash_batch(comm).tobytes() == want
        print(json.dumps({"what": "versioned_hashes", "commitments": count, "device_ms": stats(dev), "hashlib_loop_ms": round(host_ms, 3)}), flush=True)

    L = kz.lib()
    for blocks in ints(a.blocks):
        per = 4
        comm = [rng.randbytes(48) for _ in range(DISTINCT * per)]
        txs = [ec.blob_tx([ec.versioned_hash(c) for c in comm[per * k:per * k + per]], rng, dynamic=100) for k in range(DISTINCT)]
        data = np.frombuffer(b"".join(txs[j % DISTINCT] for j in range(blocks)), dtype=np.uint8)
        offsets = np.zeros(blocks + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(txs[j % DISTINCT]) for j in range(blocks)], dtype=np.uint64)
        flat = np.frombuffer(b"".join(b"".join(comm[per * (j % DISTINCT):per * (j % DISTINCT) + per]) for j in range(blocks)), dtype=np.uint8)
        tx_counts, comm_counts = np.ones(blocks, dtype=np.uint64), np.full(blocks, per, dtype=np.uint64)
        out = np.zeros(blocks, dtype=np.uint8)
        p = lambda arr: arr.ctypes.data_as(C.c_void_p)

        def call():
            assert L.kzg_hip_eth_verify_kzg_commitments_against_transactions_batch(eth.h, p(data), p(offsets), p(tx_counts), p(flat), p(comm_counts), blocks, p(out)) == 0
        ts = times(call, a.reps)
        assert (out == 1).all()
        print(json.dumps({"what": "commitments_against_transactions", "blocks": blocks, "blobs_per_block": per, "call_ms": stats(ts)}), flush=True)
    eth.close(); fs.close()


if __name__ == "__main__":
    main()
