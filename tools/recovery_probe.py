"""Erasure recovery timings.  Without --batch: the lone calls' latency per scale.  With --batch: profiles/recovery_batch.md -- per n in {4096, 32768}, half of the
samples missing, batch in {1, 16, 64, 256}: whole-call time over rows of the batch call (per-row masks, shared mask) against a sequential loop of lone calls and
lone calls from 16 threads, and the same for the vanishing polynomial alone in both constructions.  One process; every shape is warmed up; every window is a host
clock around blocking calls (each ends in a stream synchronise) and lasts at least 0.4 s."""
import argparse
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import gokzg_amd as kz


def lone_latency(scales):
    for scale in scales:
        n = 1 << scale
        fs = kz.FFTSettings(scale)
        poly, _ = fs.fr_from_32(bench.splitmix_blobs_le32(3, 1, n).reshape(-1, 32))
        poly[n // 2:] = 0
        data = fs.fft(poly, False)
        rng = np.random.default_rng(1)
        present = np.ones(n, dtype=np.uint8); present[rng.permutation(n)[: n // 2]] = 0
        samples = data.copy(); samples[present == 0] = 0
        missing = np.nonzero(present == 0)[0]
        fs.zero_poly_via_multiplication(missing, n)
        t0 = time.time(); fs.zero_poly_via_multiplication(missing, n); t1 = time.time()
        out = fs.recover_poly_from_samples(samples, present); t2 = time.time()
        out = fs.recover_poly_from_samples(samples, present); t3 = time.time()
        print("scale %d: zero_poly %.2f ms, recover %.2f ms, exact %s" % (scale, (t1 - t0) * 1e3, (t3 - t2) * 1e3, bool(np.array_equal(out, data))))
        fs.close()


def timed(fn, window=0.4):
    """seconds per call of fn(): one warm-up call, then whole calls until the window is full"""
    fn()
    reps, t0 = 0, time.perf_counter()
    while True:
        fn(); reps += 1
        dt = time.perf_counter() - t0
        if dt >= window:
            return dt / reps


def threaded(fn, rows, threads=16):
    """seconds per row when `threads` threads share `rows` lone calls (ctypes releases the GIL for the call)"""
    def run():
        def work(t):
            for r in range(t, rows, threads):
                fn(r)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    return timed(run) / rows


def with_env(value, fn):
    def run():
        old = os.environ.get("KZG_HIP_ZERO_POLY")
        os.environ["KZG_HIP_ZERO_POLY"] = value                      # read per call by the batch path
        try:
            return fn()
        finally:
            if old is None:
                del os.environ["KZG_HIP_ZERO_POLY"]
            else:
                os.environ["KZG_HIP_ZERO_POLY"] = old
    return run


def batch_profile(out_path, sizes=(4096, 32768), batches=(1, 16, 64, 256)):
    lines = ["# Batched erasure recovery: whole-call time over rows", "",
             "`python tools/recovery_probe.py --batch`: one process, half of the samples of every row missing (different places per row), host buffers, every shape warmed up,",
             "host clock around blocking calls, windows of at least 0.4 s.  All figures are microseconds per row: the time of the whole call (or loop) divided by its rows.", ""]
    for n in sizes:
        fs = kz.FFTSettings(n.bit_length() - 1)
        rows = max(batches)
        rng = np.random.default_rng(n)
        polys, _ = fs.fr_from_32(bench.splitmix_blobs_le32(5, rows, n).reshape(-1, 32))
        polys = polys.reshape(rows, n, 4)
        polys[:, n // 2:] = 0
        data = fs.fft_batch(polys)
        present = np.ones((rows, n), dtype=np.uint8)
        for r in range(rows):
            present[r, rng.permutation(n)[: n // 2]] = 0
        samples = data.copy(); samples[present == 0] = 0
        shared = data.copy(); shared[:, present[0] == 0] = 0
        lists = [np.nonzero(present[r] == 0)[0].astype(np.uint64) for r in range(rows)]
        out, status = fs.recover_poly_from_samples_batch(samples, present)
        assert not status.any() and np.array_equal(out, data), "batch recovery is wrong"
        assert np.array_equal(fs.recover_poly_from_samples_batch(shared, present[0])[0], data), "shared-mask recovery is wrong"
        lone_rec = lambda r: fs.recover_poly_from_samples(samples[r], present[r])
        lone_zero = lambda r: fs.zero_poly_via_multiplication(lists[r], n)
        seq_rows = 16
        seq_rec = timed(lambda: [lone_rec(r) for r in range(seq_rows)]) / seq_rows
        seq_zero = timed(lambda: [lone_zero(r) for r in range(seq_rows)]) / seq_rows
        thr_rec, thr_zero = threaded(lone_rec, 64), threaded(lone_zero, 64)
        lines += ["## n = %d" % n, "", "Lone calls: recovery %.1f us per row in a sequential loop, %.1f from 16 threads; zero polynomial %.1f sequential, %.1f from 16 threads." %
                  (seq_rec * 1e6, thr_rec * 1e6, seq_zero * 1e6, thr_zero * 1e6), "",
                  "| batch | recover, per-row masks | recover, shared mask | loop / batch | zero poly, direct | zero poly, tree | zero poly, default |", "|---|---|---|---|---|---|---|"]
        for b in batches:
            rec = timed(lambda: fs.recover_poly_from_samples_batch(samples[:b], present[:b])) / b
            sh = timed(lambda: fs.recover_poly_from_samples_batch(shared[:b], present[0])) / b
            zd = timed(with_env("direct", lambda: fs.zero_poly_via_multiplication_batch(lists[:b], n))) / b
            zt = timed(with_env("tree", lambda: fs.zero_poly_via_multiplication_batch(lists[:b], n))) / b
            zz = timed(lambda: fs.zero_poly_via_multiplication_batch(lists[:b], n)) / b
            lines.append("| %d | %.1f | %.1f | %.1fx | %.1f | %.1f | %.1f |" % (b, rec * 1e6, sh * 1e6, seq_rec / rec, zd * 1e6, zt * 1e6, zz * 1e6))
            print(lines[-1], flush=True)
        lines.append("")
        fs.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="store_true", help="write the batch profile instead of printing lone latencies")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "recovery_batch.md"))
    ap.add_argument("scales", nargs="*", type=int)
    args = ap.parse_args()
    if args.batch:
        batch_profile(args.out)
    else:
        lone_latency(args.scales or (12, 16))
