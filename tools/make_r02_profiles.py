#!/usr/bin/env python3
"""Builds profiles/r02_pmc.json and profiles/r02_kernel_stats.md from the output of tools/profile_round2.sh
(gpurun_out/prof_r02/{pmc_rows.jsonl, kernel_stats.md, bench_line.json})."""
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(R, "gpurun_out", sys.argv[1] if len(sys.argv) > 1 else "prof_r02")
rows = [json.loads(l) for l in open(os.path.join(src, "pmc_rows.jsonl"))]
bl = json.load(open(os.path.join(src, "bench_line.json")))
ks = open(os.path.join(src, "kernel_stats.md")).read()
CTRS = ("FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU", "GRBM_GUI_ACTIVE", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_BUSY_CYCLES", "SQ_WAVES")


def get(k, c):
    return next(r for r in rows if r["kernel"] == k and r["counter"] == c)


fb = {c: get("k_fb_accumulate", c)["avg_per_launch"] for c in CTRS}
fk = {c: get("k_g1_fft_stage", c)["avg_per_launch"] for c in CTRS}
L = bl["roofline_fk20"]["launches_per_step"]
pm = {
    "source": "rocprofv3 --pmc <one counter per pass> --kernel-trace --output-format csv (tools/profile_round2.sh r02), 1x MI355X; FETCH_SIZE / WRITE_SIZE in KiB as reported, raw values (the guide's x2 correction applies to wide coalesced streams; these kernels gather 96- and 104-byte records); SQ_INSTS_VALU counts wave64 instructions; SQ_WAIT_* / SQ_ACTIVE_* count quad-cycles summed over waves; GRBM_GUI_ACTIVE is summed over the 8 XCDs",
    "k_fb_accumulate": {"kernel": "k_fb_accumulate", "batch": 512, "n": 4096, "table_c": 16, "table_windows": 16, "lanes": 131072,
                        "fetch_bytes_per_launch": fb["FETCH_SIZE"] * 1024, "write_bytes_per_launch": fb["WRITE_SIZE"] * 1024, "valu_insts_per_launch": fb["SQ_INSTS_VALU"],
                        "gui_active_cycles_per_launch_all_xcd": fb["GRBM_GUI_ACTIVE"], "sq_wait_inst_any": fb["SQ_WAIT_INST_ANY"], "sq_active_inst_any": fb["SQ_ACTIVE_INST_ANY"],
                        "sq_busy_cycles": fb["SQ_BUSY_CYCLES"], "waves": fb["SQ_WAVES"], "scratch_bytes_per_lane": get("k_fb_accumulate", "SQ_WAVES")["scratch_bytes_per_lane"],
                        "lds_bytes_per_workgroup": get("k_fb_accumulate", "SQ_WAVES")["lds"], "vgprs": 256},
    "k_g1_fft_stage": {"kernel": "k_g1_fft_stage (+ k_g1_fft_stage_dif)", "batch": 512, "n": 4096, "launches_per_step": L,
                       "fetch_bytes_per_step": fk["FETCH_SIZE"] * 1024 * L, "write_bytes_per_step": fk["WRITE_SIZE"] * 1024 * L, "valu_insts_per_step": fk["SQ_INSTS_VALU"] * L,
                       "gui_active_cycles_per_launch_all_xcd": fk["GRBM_GUI_ACTIVE"], "sq_wait_inst_any": fk["SQ_WAIT_INST_ANY"], "sq_active_inst_any": fk["SQ_ACTIVE_INST_ANY"],
                       "sq_busy_cycles": fk["SQ_BUSY_CYCLES"], "waves_per_launch": fk["SQ_WAVES"], "scratch_bytes_per_lane": get("k_g1_fft_stage", "SQ_WAVES")["scratch_bytes_per_lane"],
                       "lds_bytes_per_workgroup": 0, "vgprs": 256},
}
json.dump(pm, open(os.path.join(R, "profiles", "r02_pmc.json"), "w"), indent=1)
f, k = pm["k_fb_accumulate"], pm["k_g1_fft_stage"]
mads_fb = 512 * 4096 * 16 * 3055
mads_fk = 512 * bl["roofline_fk20"]["mac"]["mads_per_all_proofs"]
cal_mad = bl["roofline"]["mac"]["measured_peak_Tmad_s"] * 1e12
cal_add = bl["roofline"]["mac"]["measured_v_add_u32_Tops_s"] * 1e12
t_fb = bl["roofline"]["avg_launch_ms"] * 1e-3
t_fk = bl["roofline_fk20"]["avg_launch_ms"] * L * 1e-3


def model(mads, insts):
    return mads / cal_mad + (insts * 64 - mads) / cal_add


doc = f"""# r02 — kernel statistics and counters at the end of round 2 (1x MI355X)

State: round-1 kernels + table walk in 256-lane workgroups with a wave-cooperative block tree and finish (windows of a point divided
among up to 8 lanes below 32 polynomials), GLV bucket MSM with scan reduce and wave-cooperative Horner for caller-supplied points,
direct radix-16 / radix-8 passes for 1-4 G1 transforms, request coalescing of one-polynomial calls; G1 FFT stages (256-lane workgroups)
with an affine width-5 NAF table built by co-Z arithmetic (one inversion per multiplication, mixed additions) and precomputed digit
rows, the regular odd-digit schedule on the same table where wavefronts straddle twiddles; FK20: Toeplitz stage fused with the first
two decimation-in-frequency stages of the inverse transform ({L} stage launches per step).

Commands (GPU box): `bash tools/profile_round2.sh r02` =
`cd /tmp && rocprofv3 --kernel-trace --stats -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extras` (summary by
`tools/rocprof_summary.py`), then ONE `rocprofv3 --pmc <counter> --kernel-trace --output-format csv` pass per counter and per kernel
(`bench.py --full --no-fk20` for `k_fb_accumulate`: every launch 512 blobs; `bench.py --full --no-extras --fk20-multi-batch 0` for the stage kernels
`k_g1_fft_stage` / `k_g1_fft_stage_dif`, launches of the 512-polynomial FK20 step selected by grid size), then the un-profiled bench line;
`tools/make_r02_profiles.py` writes this file and `r02_pmc.json`.  `k_fb_build_*`, `k_msm_window_rows`, `k_g1_to_affine`,
`k_g1_fixed_base_powers`, `k_g1_decompress` are one-time settings construction; `k_cal_*` is the in-run calibration.

{ks}

## Counters (separate `--pmc` passes; raw values in `profiles/r02_pmc.json`)

| | `k_fb_accumulate` (512 blobs, c = 16, per launch) | G1 FFT stage kernels (512 polynomials, per step of {L} launches) |
|---|---|---|
| HIP-event time (un-profiled bench, same box) | {t_fb*1e3:.2f} ms | {t_fk*1e3:.1f} ms ({bl['roofline_fk20']['avg_launch_ms']:.1f} ms per launch) |
| algorithmic bytes (SURVEY 8d) | 67.6 MB | 436 MB (512 x 851 968 B) |
| FETCH_SIZE / WRITE_SIZE | {f['fetch_bytes_per_launch']/1e9:.2f} GB / {f['write_bytes_per_launch']/1e6:.0f} MB | {k['fetch_bytes_per_step']/1e9:.0f} GB / {k['write_bytes_per_step']/1e9:.0f} GB |
| = HBM rate | {(f['fetch_bytes_per_launch']+f['write_bytes_per_launch'])/t_fb/1e12:.2f} TB/s | {(k['fetch_bytes_per_step']+k['write_bytes_per_step'])/t_fk/1e12:.2f} TB/s |
| SQ_INSTS_VALU (wave64) | {f['valu_insts_per_launch']:.3e} | {k['valu_insts_per_step']:.3e} |
| of which `v_mad_u64_u32` (analytic, DESIGN.md 4) | {mads_fb/64:.3e} ({mads_fb/64/f['valu_insts_per_launch']*100:.0f} %) | {mads_fk/64:.3e} ({mads_fk/64/k['valu_insts_per_step']*100:.0f} %) |
| SQ_WAIT_INST_ANY / SQ_ACTIVE_INST_ANY | {f['sq_wait_inst_any']/f['sq_active_inst_any']:.2f} | {k['sq_wait_inst_any']/k['sq_active_inst_any']:.2f} |
| clock while the kernel runs (GRBM_GUI_ACTIVE / 8 XCDs / time) | {f['gui_active_cycles_per_launch_all_xcd']/8/t_fb/1e9:.2f} GHz | {k['gui_active_cycles_per_launch_all_xcd']/8/(t_fk/L)/1e9:.2f} GHz |
| multiply-add rate vs the rate measured in the same run ({cal_mad/1e12:.1f} T/s) | {mads_fb/t_fb/1e12:.1f} T/s = **{mads_fb/t_fb/cal_mad:.2f}** | {mads_fk/t_fk/1e12:.1f} T/s = **{mads_fk/t_fk/cal_mad:.2f}** |
| issue model: mads / mad rate + other VALU / `v_add_u32` rate ({cal_add/1e12:.1f} T/s) | {model(mads_fb,f['valu_insts_per_launch'])*1e3:.2f} ms = {model(mads_fb,f['valu_insts_per_launch'])/t_fb*100:.0f} % of the launch | {model(mads_fk,k['valu_insts_per_step'])*1e3:.0f} ms = {model(mads_fk,k['valu_insts_per_step'])/t_fk*100:.0f} % of the step |
| VGPRs / scratch per lane / LDS per workgroup | 256 / {f['scratch_bytes_per_lane']} B / {f['lds_bytes_per_workgroup']} B | 256 / {k['scratch_bytes_per_lane']} B / 0 |

Bench line of the profiled box: {bl['value']:.0f} commitments/s, {bl['fk20']['value']:.0f} FK20 all-proofs/s, {bl['fk20_multi']['value']:.0f} FK20Multi/s.

Reading.

* Both kernels are **instruction-issue bound**, not HBM bound.  With the instruction mix they execute, pure issue at the rates measured
  on this GPU accounts for {model(mads_fb,f['valu_insts_per_launch'])/t_fb*100:.0f} % (table walk) and {model(mads_fk,k['valu_insts_per_step'])/t_fk*100:.0f} % (FFT stages) of their time; the table walk additionally runs at a lower clock
  (power: it streams 0.6 TB/s of gathers while multiplying).  `SQ_WAIT_INST_ANY` is high in both because a SIMD with two
  resident waves always has one of them waiting for the issue port the other is using; it is not idle time.
* The walk's traffic (3.3 GB per launch, 50x the algorithmic bytes) is the design: one 96-byte gather per mixed addition out of a
  206 GB table buys 16 additions per coefficient instead of ~29 plus doublings.  It is 7 % of HBM bandwidth.
* The FFT stages' traffic ({k['fetch_bytes_per_step']/512/1e9:.2f} GB fetched + {k['write_bytes_per_step']/512/1e9:.2f} GB written per FK20) is private scratch of the scalar multiplication
  (the Jacobian multiples while the table is built, the 8-entry affine table, spills of the out-of-line table-building code).  It is
  ~10 % of HBM bandwidth and hidden: the kernels sit at {model(mads_fk,k['valu_insts_per_step'])/t_fk*100:.0f} % of their issue bound.
* What helps is fewer instructions per group operation.  Round 2 removed ~10 % of the FK20 multiply-adds (mixed additions from an affine
  table; two stages of the inverse transform moved into the fixed-base Toeplitz stage); `profiles/r02_valu_calibration.md` shows where
  the instructions of a product go (67 % multiplies, 19 % 64-bit carry arithmetic that issues at multiply rate, 14 % masks / moves) and
  why no cheaper multiplier exists on this ISA.  Commitments: **{mads_fb/t_fb/cal_mad:.2f} of the multiply roof**; 100 k/s would need 0.70.
  FK20: **{mads_fk/t_fk/cal_mad:.2f} of the multiply roof**.
"""
open(os.path.join(R, "profiles", "r02_kernel_stats.md"), "w").write(doc)
print(doc[-2600:])
