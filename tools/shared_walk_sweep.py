#!/usr/bin/env python3
"""Crossovers of the shared-window walk (FB_SHARED_MIN_BATCH, FB_SHARED_MIN_BATCH_REPLACED in go-kzg_amd/csrc/capi_kzg.hip): ms per
kzg_hip_commit_to_poly_batch_dev step on device-resident blobs, one process, four handles on the 4096-point setup:
    windows16 : the all-window table of the default budget (c = 16, 103 GB), KZG_HIP_FB_LAYOUT=windows -- the walk every batch took before
    windows11 : the all-window table a handle keeps beside a shared table of the whole default budget (c = 11, 4.8 GB)
    shared    : the single-point shared-window table of the default budget (c = 19, 103 GB), forced at every batch size
    paired    : the paired-point table of the default budget (10-bit digits of two neighbouring points, 103 GB, 13 additions), forced at every batch size
Prints median and spread (max - min) of the timed steps per batch size and checks that the four agree on the commitments.
usage: python tools/shared_walk_sweep.py [steps]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
import gokzg_amd as kz  # noqa: E402
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
sizes = (32, 64, 128, 256, 512, 1024, 2048, 4096)
lib = kz.lib()
fs = kz.FFTSettings(12)
raw = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g1.bin"), "rb").read(), dtype=np.uint8)
setup = fs.from_compressed_g1(raw)
blobs, _ = fs.fr_from_32(bench.splitmix_blobs_le32(1, max(sizes), 4096).reshape(-1, 32))
d_in = torch.from_numpy(blobs.reshape(max(sizes), 4096, 4).view(np.int64)).cuda()
s = torch.cuda.current_stream().cuda_stream


def run(ks, env, B):
    for k in ("KZG_HIP_FB_LAYOUT", "KZG_HIP_FB_SHARED_MIN_BATCH"):
        os.environ.pop(k, None)
    os.environ.update(env)
    d_out = torch.zeros((B, 18), dtype=torch.int64, device="cuda")
    ts = []
    for i in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = lib.kzg_hip_commit_to_poly_batch_dev(ks.h, d_in.data_ptr(), 4096, B, d_out.data_ptr(), s)
        torch.cuda.synchronize()
        assert st == 0, st
        if i >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), max(ts) - min(ts), d_out.cpu().numpy()


legs = (("windows16", 110.0, {"KZG_HIP_FB_LAYOUT": "windows"}), ("windows11", 6.0, {"KZG_HIP_FB_LAYOUT": "windows"}),
        ("shared", 110.0, {"KZG_HIP_FB_LAYOUT": "shared", "KZG_HIP_FB_SHARED_MIN_BATCH": "1"}),
        ("paired", 110.0, {"KZG_HIP_FB_LAYOUT": "paired", "KZG_HIP_FB_SHARED_MIN_BATCH": "1"}))
res, outs = {}, {}
for name, gb, env in legs:
    ks = kz.KZGSettings(fs, setup)
    ks.set_table_budget_gb(gb)
    t0 = time.perf_counter()
    run(ks, env, 64)
    print("%s: table %s, %d additions per coefficient, first call %.1f s" % (name, ks.table_info(), ks.table_additions(), time.perf_counter() - t0), flush=True)
    for B in sizes:
        med, spread, out = run(ks, env, B)
        res[name, B] = (med, spread)
        outs[name, B] = out
    ks.close()
print("| blobs | windows16 ms (spread) | windows11 ms (spread) | shared ms (spread) | paired ms (spread) | shared / windows16 | shared / windows11 | paired / shared |")
print("|---|---|---|---|---|---|---|---|")
for B in sizes:
    a, b, c, d = res["windows16", B], res["windows11", B], res["shared", B], res["paired", B]
    assert np.array_equal(outs["windows16", B], outs["shared", B]) and np.array_equal(outs["windows11", B], outs["shared", B]) and np.array_equal(outs["paired", B], outs["shared", B]), B
    print("| %d | %.3f (%.3f) | %.3f (%.3f) | %.3f (%.3f) | %.3f (%.3f) | %.3f | %.3f | %.3f |" % (B, a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1], c[0] / a[0], c[0] / b[0], d[0] / c[0]), flush=True)
