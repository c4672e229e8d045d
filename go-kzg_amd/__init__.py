"""go-kzg_amd -- host-side mirror of go-kzg's FFTSettings / KZGSettings / FK20*Settings API over libkzg_hip.so.

The reference's host language is Go, which this image does not have; the drop-in boundary is the C ABI in
include/kzg_hip.h (the cgo shim for it is in go-kzg_amd/goshim/ and INTEGRATION.md).  This module is the same
thin binding written with ctypes so that the parity tests read like the reference's own tests:

    fs = FFTSettings(4)                         # kzg.NewFFTSettings(4)              fft.go:44
    ks = KZGSettings(fs, secret_g1)             # kzg.NewKZGSettings(fs, s1, s2)     kzg.go:21
    c  = ks.commit_to_poly(poly)                # ks.CommitToPoly(poly)              kzg_single_proofs.go:17
    fk = FK20SingleSettings(ks, 32)             # kzg.NewFK20SingleSettings(ks, 32)  kzg.go:43
    pr = fk.da_using_fk20(poly)                 # fk.DAUsingFK20(poly)               fk20_single.go:176

Values are numpy uint64 arrays holding the memory images of the reference's default backend:
Fr -> (n, 4) Montgomery limbs; G1 -> (n, 3, 6) Jacobian Montgomery limbs (inf <=> Z == 0).

There is NO CPU fallback: importing works anywhere (so the C ABI can be inspected), but constructing
FFTSettings without a gfx950 device raises NoDeviceError, and a missing libkzg_hip.so raises ImportError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KZG_HIP_LIB") or os.path.join(_HERE, "libkzg_hip.so")   # KZG_HIP_LIB: another build of the same library (A/B runs)

OK, ERR_TOO_WIDE, ERR_NOT_POW2, ERR_LEN_MISMATCH, ERR_UPPER_HALF, ERR_BAD_ARG, ERR_BAD_POINT, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_RECOVERY, ERR_BAD_BLOB = range(12)


class KzgError(Exception):
    """The reference returns an `error` (fft_fr.go:57-59,78-83; fft_g1.go:60-65)."""

    def __init__(self, status, msg=""):
        super().__init__("kzg_hip status %d %s" % (status, msg))
        self.status = status


class KzgPanic(KzgError):
    """The reference panics (kzg.go:22-27,44-52,74-91; fk20_single.go:60-62,140-154; bls_kilic.go:133-135)."""


class NoDeviceError(KzgError):
    pass


_lib = None


def lib():
    """Loads libkzg_hip.so (built by `make -C go-kzg_amd/csrc` / __graft_entry__.build()); fails loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libkzg_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback: " + LIB_PATH)
    if os.environ.get("KZG_HIP_NO_TORCH_PRELOAD") != "1":
        # PyTorch bundles its own libamdhip64; if this library initialises /opt/rocm's copy first, torch later reports
        # "No HIP GPUs are available".  Importing torch first makes both resolve to ONE HIP runtime (same SONAME).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, u64, i32, u32 = C.c_void_p, C.c_uint64, C.c_int, C.c_uint
    pp = C.POINTER(C.c_void_p)
    sig = {
        "kzg_hip_device_count": (i32, []), "kzg_hip_last_error": (C.c_char_p, []), "kzg_hip_version": (C.c_char_p, []),
        "kzg_hip_host_register": (i32, [vp, u64]), "kzg_hip_host_unregister": (i32, [vp]),
        "kzg_hip_fft_settings_new": (i32, [i32, u32, pp]), "kzg_hip_fft_settings_free": (None, [vp]),
        "kzg_hip_fft_max_width": (u64, [vp]), "kzg_hip_fft_roots": (i32, [vp, i32, vp]),
        "kzg_hip_fft_fr": (i32, [vp, vp, u64, i32, vp, C.POINTER(u64)]), "kzg_hip_inplace_fft_fr": (i32, [vp, vp, vp, u64, i32]),
        "kzg_hip_fft_fr_batch": (i32, [vp, vp, u64, u64, i32, vp]), "kzg_hip_fft_g1": (i32, [vp, vp, u64, i32, vp]),
        "kzg_hip_fft_g1_batch": (i32, [vp, vp, u64, u64, i32, vp]), "kzg_hip_multi_fft_g1_batch": (i32, [vp, vp, u64, u64, i32, vp]),
        "kzg_hip_das_fft_extension": (i32, [vp, vp, u64]), "kzg_hip_das_fft_extension_batch": (i32, [vp, vp, u64, u64]),
        "kzg_hip_fft_fr_batch_dev": (i32, [vp, vp, u64, u64, i32, vp, vp]), "kzg_hip_fft_g1_batch_dev": (i32, [vp, vp, u64, u64, i32, vp, vp]),
        "kzg_hip_das_fft_extension_batch_dev": (i32, [vp, vp, u64, u64, vp]),
        "kzg_hip_fr_from_le32": (i32, [vp, vp, u64, vp, C.POINTER(i32)]), "kzg_hip_fr_to_le32": (i32, [vp, vp, u64, vp]),
        "kzg_hip_lincomb_g1": (i32, [vp, vp, vp, u64, vp]),
        "kzg_hip_points_new": (i32, [vp, vp, u64, pp]), "kzg_hip_points_free": (None, [vp]), "kzg_hip_points_count": (u64, [vp]),
        "kzg_hip_points_set_table_budget_gb": (i32, [vp, C.c_double]),
        "kzg_hip_lincomb_points": (i32, [vp, vp, u64, vp]), "kzg_hip_lincomb_points_batch": (i32, [vp, vp, u64, u64, vp]),
        "kzg_hip_lincomb_points_batch_dev": (i32, [vp, vp, u64, u64, vp, vp]), "kzg_hip_g1_to_compressed": (i32, [vp, vp, u64, vp]),
        "kzg_hip_g1_from_compressed": (i32, [vp, vp, u64, vp]), "kzg_hip_g1_mul_vec": (i32, [vp, vp, vp, u64, vp]),
        "kzg_hip_generate_testing_setup_g1": (i32, [vp, vp, u64, vp]),
        "kzg_hip_g1_marshal_text": (i32, [vp, vp, u64, vp]), "kzg_hip_g1_unmarshal_text": (i32, [vp, C.c_char_p, u64, vp]),
        "kzg_hip_trusted_setup_from_json": (i32, [vp, C.c_char_p, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]),
        "kzg_hip_kzg_set_table_budget_gb": (i32, [vp, C.c_double]),
        "kzg_hip_kzg_settings_new": (i32, [vp, vp, u64, pp]), "kzg_hip_kzg_settings_free": (None, [vp]),
        "kzg_hip_commit_to_poly": (i32, [vp, vp, u64, vp]), "kzg_hip_commit_to_poly_batch": (i32, [vp, vp, u64, u64, vp]),
        "kzg_hip_commit_to_poly_batch_dev": (i32, [vp, vp, u64, u64, vp, vp]),
        "kzg_hip_compute_proof_single": (i32, [vp, vp, u64, u64, vp]),
        "kzg_hip_compute_proof_single_batch": (i32, [vp, vp, u64, u64, vp, vp]),
        "kzg_hip_compute_proof_single_batch_dev": (i32, [vp, vp, u64, u64, vp, vp, vp]),
        "kzg_hip_compute_proof_multi": (i32, [vp, vp, u64, u64, u64, vp]),
        "kzg_hip_check_proof_multi_interpolation": (i32, [vp, vp, u64, vp, vp, vp]),
        "kzg_hip_g2_from_compressed": (i32, [vp, vp, u64, vp]), "kzg_hip_pairings_verify_batch": (i32, [vp, vp, vp, vp, vp, u64, vp]),
        "kzg_hip_g2_mul_generator_vec": (i32, [vp, vp, u64, vp]), "kzg_hip_generate_testing_setup_g2": (i32, [vp, vp, u64, vp]),
        "kzg_hip_g2_to_compressed": (i32, [vp, vp, u64, vp]),
        "kzg_hip_trusted_setup_g2_from_json": (i32, [vp, C.c_char_p, u64, vp, u64, C.POINTER(u64)]),
        "kzg_hip_test_g2_table_builds": (i32, [vp, C.POINTER(u64)]),
        "kzg_hip_kzg_set_secret_g2": (i32, [vp, vp, u64]), "kzg_hip_check_proof_single_batch": (i32, [vp, vp, vp, vp, vp, u64, vp]),
        "kzg_hip_check_proof_multi_batch": (i32, [vp, vp, vp, vp, vp, u64, u64, vp]),
        "kzg_hip_check_proof_single_batch_combined": (i32, [vp, vp, vp, vp, vp, u64, vp, vp]),
        "kzg_hip_eth_verify_kzg_proof_batch_combined": (i32, [vp, vp, vp, vp, vp, u64, vp, vp]),
        "kzg_hip_test_combine_points": (i32, [vp, vp, vp, vp, vp, u64, vp, vp, vp]), "kzg_hip_test_combine_stats": (i32, [C.POINTER(u64)]),
        "kzg_hip_check_proof_multi_batch_combined": (i32, [vp, vp, vp, vp, vp, u64, u64, vp, vp]),
        "kzg_hip_test_combine_multi_points": (i32, [vp, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp]), "kzg_hip_test_combine_multi_route": (i32, [u64, u64, C.POINTER(u64)]),
        "kzg_hip_eth_set_setup_g2": (i32, [vp, vp, u64]), "kzg_hip_eth_verify_kzg_proof_batch": (i32, [vp, vp, vp, vp, vp, u64, vp]),
        "kzg_hip_eth_verify_aggregate_kzg_proof_batch": (i32, [vp, vp, vp, vp, vp, u64, vp, vp, vp, vp]),
        "kzg_hip_eth_kzg_to_versioned_hash_batch": (i32, [vp, vp, u64, vp]), "kzg_hip_eth_kzg_to_versioned_hash_batch_dev": (i32, [vp, vp, u64, vp]),
        "kzg_hip_eth_point_evaluation_precompile_batch": (i32, [vp, vp, u64, vp]),
        "kzg_hip_eth_point_evaluation_precompile_batch_dev": (i32, [vp, vp, u64, vp]),
        "kzg_hip_eth_precompile_return_value": (i32, [vp, vp]),
        "kzg_hip_eth_verify_kzg_commitments_against_transactions_batch": (i32, [vp, vp, vp, vp, vp, vp, u64, vp]),
        "kzg_hip_test_sha256_lanes": (i32, [vp, vp, vp, vp, u64, vp]), "kzg_hip_test_hash_to_bls_field_lanes": (i32, [vp, vp, u64, vp]),
        "kzg_hip_pairing_test": (i32, [vp, vp, vp, u64, vp]),
        "kzg_hip_pairing_test_wave": (i32, [vp, vp, vp, u64, vp]), "kzg_hip_test_wave_fp12_op": (i32, [vp, i32, vp, vp, u64, vp]),
        "kzg_hip_test_pairing_route": (i32, [u64, C.POINTER(u64)]),
        "kzg_hip_toeplitz_part2": (i32, [vp, vp, vp, u64, vp]), "kzg_hip_toeplitz_part3": (i32, [vp, vp, u64, vp]),
        "kzg_hip_fk20_single_settings_new": (i32, [vp, u64, pp]), "kzg_hip_fk20_single_settings_free": (None, [vp]),
        "kzg_hip_fk20_single_x_ext_fft": (i32, [vp, vp]), "kzg_hip_fk20_single": (i32, [vp, vp, u64, vp]),
        "kzg_hip_fk20_single_batch": (i32, [vp, vp, u64, u64, vp]), "kzg_hip_fk20_single_batch_dev": (i32, [vp, vp, u64, u64, vp, vp]),
        "kzg_hip_fk20_single_da_optimized": (i32, [vp, vp, u64, vp]), "kzg_hip_da_using_fk20": (i32, [vp, vp, u64, vp]),
        "kzg_hip_da_using_fk20_batch": (i32, [vp, vp, u64, u64, vp]), "kzg_hip_da_using_fk20_batch_dev": (i32, [vp, vp, u64, u64, vp, vp]),
        "kzg_hip_fk20_multi_settings_new": (i32, [vp, u64, u64, pp]), "kzg_hip_fk20_multi_settings_free": (None, [vp]),
        "kzg_hip_fk20_multi": (i32, [vp, vp, u64, vp]), "kzg_hip_fk20_multi_da_optimized": (i32, [vp, vp, u64, vp]),
        "kzg_hip_da_using_fk20_multi": (i32, [vp, vp, u64, vp]),
        "kzg_hip_da_using_fk20_multi_batch_dev": (i32, [vp, vp, u64, u64, vp, vp]),
        "kzg_hip_fk20_multi_hext_slice_dev": (i32, [vp, vp, u64, u64, u64, vp, vp]),
        "kzg_hip_fk20_multi_finish_dev": (i32, [vp, vp, i32, vp, vp]),
        "kzg_hip_eth_settings_new": (i32, [vp, vp, u64, pp]), "kzg_hip_eth_settings_free": (None, [vp]),
        "kzg_hip_eth_blob_to_kzg_commitment_batch": (i32, [vp, vp, u64, vp, vp]),
        "kzg_hip_eth_compute_kzg_proof": (i32, [vp, vp, u64, vp, vp, vp]),
        "kzg_hip_eth_compute_kzg_proof_batch": (i32, [vp, vp, u64, u64, vp, vp, vp, vp]),
        "kzg_hip_eth_compute_kzg_proof_batch_dev": (i32, [vp, vp, u64, u64, vp, vp, vp, vp, vp]),
        "kzg_hip_eth_compute_aggregate_kzg_proof": (i32, [vp, vp, u64, vp, vp]),
        "kzg_hip_eth_compute_aggregate_kzg_proof_batch": (i32, [vp, vp, vp, u64, vp, vp, vp]),
        "kzg_hip_eth_compute_aggregate_kzg_proof_batch_dev": (i32, [vp, vp, vp, u64, vp, vp, vp]),
        "kzg_hip_test_eth_prove_chunks": (u64, []),
        "kzg_hip_eth_compute_aggregated_poly_and_commitment": (i32, [vp, vp, vp, u64, vp, vp, vp, vp]),
        "kzg_hip_test_sha256": (None, [vp, u64, vp]),
        "kzg_hip_evaluate_poly_in_evaluation_form": (i32, [vp, vp, u64, vp, u32, vp]),
        "kzg_hip_eth_evaluate_polynomial_in_evaluation_form": (i32, [vp, vp, u64, vp, vp]),
        "kzg_hip_bench_threads_fft_fr": (i32, [vp, vp, u64, u64, u32, u32, vp, C.POINTER(C.c_double)]),
        "kzg_hip_bench_drop_in_eth_proof": (i32, [vp, vp, u64, u64, u32, u32, vp, C.POINTER(C.c_double)]),
        "kzg_hip_zero_poly_via_multiplication": (i32, [vp, vp, u64, u64, vp, vp]),
        "kzg_hip_recover_poly_from_samples": (i32, [vp, vp, vp, u64, vp]),
        "kzg_hip_recover_poly_from_samples_batch": (i32, [vp, vp, vp, u64, u64, u64, vp, vp]),
        "kzg_hip_recover_poly_from_samples_batch_dev": (i32, [vp, vp, vp, u64, u64, u64, vp, vp, vp]),
        "kzg_hip_zero_poly_via_multiplication_batch": (i32, [vp, vp, vp, u64, u64, vp, vp, vp]),
        "kzg_hip_calibrate": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "kzg_hip_bench_drop_in": (i32, [vp, i32, vp, u64, u64, u32, u32, vp, C.POINTER(C.c_double)]),
        "kzg_hip_coalesce_stats": (i32, [vp, i32, C.POINTER(u64)]),
        "kzg_hip_lincomb_promotions": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "kzg_hip_test_fp_inv": (i32, [vp, vp, u64, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "kzg_hip_test_fr_inv": (i32, [vp, vp, u64, vp, vp, vp]),
        "kzg_hip_test_g1_fft_plan": (i32, [vp, u64, u64, u64, i32, vp]),
        "kzg_hip_test_g1_fft_stage": (i32, [vp, vp, u64, u64, u64, i32, i32, i32, i32, vp, vp]),
        "kzg_hip_test_g1_fft_direct": (i32, [vp, vp, u64, u64, u64, i32, u32, i32, u64, vp]),
        "kzg_hip_kzg_table_info": (i32, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]), "kzg_hip_kzg_table_additions": (u32, [vp]), "kzg_hip_kzg_set_projective_outputs": (i32, [vp, i32]),
        "kzg_hip_da_using_fk20_multi_batch": (i32, [vp, vp, u64, u64, vp]),
        "kzg_hip_multi_settings_new": (i32, [C.POINTER(i32), u32, u32, vp, u64, pp]), "kzg_hip_multi_settings_free": (None, [vp]),
        "kzg_hip_multi_device_count": (u32, [vp]), "kzg_hip_multi_device": (i32, [vp, u32]),
        "kzg_hip_multi_fft": (vp, [vp, u32]), "kzg_hip_multi_kzg": (vp, [vp, u32]),
        "kzg_hip_multi_transport": (C.c_char_p, [vp]), "kzg_hip_multi_transport_note": (C.c_char_p, [vp]), "kzg_hip_multi_transport_check": (C.c_char_p, [vp]), "kzg_hip_multi_exchanges": (u64, [vp]),
        "kzg_hip_multi_set_fft_sharding": (i32, [vp, i32]), "kzg_hip_multi_set_table_budget_gb": (i32, [vp, C.c_double]),
        "kzg_hip_multi_commit_to_poly_batch": (i32, [vp, vp, u64, u64, vp]),
        "kzg_hip_multi_compute_proof_single_batch": (i32, [vp, vp, u64, u64, vp, vp]),
        "kzg_hip_multi_fft_fr_batch": (i32, [vp, vp, u64, u64, i32, vp]), "kzg_hip_multi_das_fft_extension_batch": (i32, [vp, vp, u64, u64]),
        "kzg_hip_multi_eth_settings_new": (i32, [vp, vp, u64, pp]), "kzg_hip_multi_eth_settings_free": (None, [vp]),
        "kzg_hip_multi_eth_blob_to_kzg_commitment_batch": (i32, [vp, vp, u64, vp, vp]),
        "kzg_hip_multi_eth_compute_kzg_proof_batch": (i32, [vp, vp, u64, u64, vp, vp, vp, vp]),
        "kzg_hip_multi_fk20_single_settings_new": (i32, [vp, u64, pp]), "kzg_hip_multi_fk20_single_settings_free": (None, [vp]),
        "kzg_hip_multi_da_using_fk20_batch": (i32, [vp, vp, u64, u64, vp]), "kzg_hip_multi_da_using_fk20": (i32, [vp, vp, u64, vp]),
        "kzg_hip_multi_fk20_multi_settings_new": (i32, [vp, u64, u64, pp]), "kzg_hip_multi_fk20_multi_settings_free": (None, [vp]),
        "kzg_hip_multi_da_using_fk20_multi_batch": (i32, [vp, vp, u64, u64, vp]), "kzg_hip_multi_da_using_fk20_multi": (i32, [vp, vp, u64, vp]),
        "kzg_hip_bench_poly_lincomb_dev": (i32, [vp, vp, u64, vp, u64, u64, vp, vp]),
        "kzg_hip_prof_reset": (None, [vp, i32]), "kzg_hip_prof_read": (i32, [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(u64)]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("KZG_HIP_LIB_ALLOW_MISSING") and not hasattr(L, name):
            continue           # A/B runs against an older build selected with KZG_HIP_LIB (tools/ab_latency.sh)
        f = getattr(L, name)   # AttributeError here == header / library drift
        f.restype, f.argtypes = res, args
    _lib = L
    return L


API_SYMBOLS = None  # filled by tests from include/kzg_hip.h


def device_count():
    return lib().kzg_hip_device_count()


class pinned:
    """`with pinned(array):` -- the array's memory is pinned (kzg_hip_host_register) for the duration: batch calls read it in place over PCIe"""

    def __init__(self, array):
        self.a = array

    def __enter__(self):
        _chk(lib().kzg_hip_host_register(self.a.ctypes.data, self.a.nbytes))
        return self.a

    def __exit__(self, *exc):
        lib().kzg_hip_host_unregister(self.a.ctypes.data)
        return False


_ERR_STATUS = (ERR_TOO_WIDE, ERR_NOT_POW2)


def _chk(st, error_ok=False):
    if st == OK:
        return
    msg = ""
    if st == ERR_HIP:
        msg = lib().kzg_hip_last_error().decode()
    if st == ERR_NO_DEVICE:
        raise NoDeviceError(st, "no gfx950 device visible (the HIP path is the only path)")
    if error_ok and st in _ERR_STATUS:
        raise KzgError(st, msg)
    raise KzgPanic(st, msg)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _fr(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, 4)


def _g1(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, 3, 6)


def _g2(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, 3, 2, 6)


def _seed32(seed):
    """None, or the 32 bytes of a combination seed as a ctypes buffer"""
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise KzgError(ERR_LEN_MISMATCH, "a seed is 32 bytes")
    return C.c_char_p(seed)


def combine_stats():
    """test hook: what the calling thread's last _combined proof check did, and the routing now: dict(route = "combined" | "per_row", groups,
    failed, rechecked, combine_from, rows)"""
    out = (C.c_uint64 * 6)()
    _chk(lib().kzg_hip_test_combine_stats(out))
    return {"route": "combined" if out[0] else "per_row", "groups": int(out[1]), "failed": int(out[2]), "rechecked": int(out[3]),
            "combine_from": int(out[4]), "rows": int(out[5])}


def combine_multi_route(n, count):
    """test hook: ("combined" | "per_row", COMBINE_MULTI_FROM): the route of check_proof_multi_batch_combined for `count` rows of n values under
    the current environment"""
    out = (C.c_uint64 * 2)()
    _chk(lib().kzg_hip_test_combine_multi_route(n, count, out))
    return ("combined" if out[0] else "per_row"), int(out[1])


def pairing_route(n):
    """test hook: ("wave" | "lane", PAIRING_WAVE_BELOW): the kernel a batch of n pairing checks runs under the current environment"""
    out = (C.c_uint64 * 2)()
    _chk(lib().kzg_hip_test_pairing_route(n, out))
    return ("wave" if out[0] else "lane"), int(out[1])


def g2_empty(n):
    return np.zeros((n, 3, 2, 6), dtype=np.uint64)


def fr_empty(n):
    return np.zeros((n, 4), dtype=np.uint64)


def g1_empty(n):
    return np.zeros((n, 3, 6), dtype=np.uint64)


class FFTSettings:
    """kzg.FFTSettings (fft.go:34-61) with a device-resident domain."""

    def __init__(self, max_scale, device=0):
        h = C.c_void_p()
        _chk(lib().kzg_hip_fft_settings_new(device, max_scale, C.byref(h)))
        self.h, self.max_scale, self.max_width, self.device = h, max_scale, 1 << max_scale, device

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_fft_settings_free(self.h)
            self.h = None

    def expanded_roots_of_unity(self):
        out = fr_empty(self.max_width + 1)
        _chk(lib().kzg_hip_fft_roots(self.h, 0, _p(out)))
        return out

    def reverse_roots_of_unity(self):
        out = fr_empty(self.max_width + 1)
        _chk(lib().kzg_hip_fft_roots(self.h, 1, _p(out)))
        return out

    def fft(self, vals, inv=False):
        """FFTSettings.FFT (fft_fr.go:55-74)"""
        vals = _fr(vals)
        n = vals.shape[0]
        if n > self.max_width:
            raise KzgError(ERR_TOO_WIDE)
        np2 = 1 if n == 0 else 1 << (n - 1).bit_length()
        out, on = fr_empty(np2), C.c_uint64(0)
        _chk(lib().kzg_hip_fft_fr(self.h, _p(vals), n, int(inv), _p(out), C.byref(on)), error_ok=True)
        return out

    def inplace_fft(self, vals, inv=False):
        """FFTSettings.InplaceFFT (fft_fr.go:76-105); returns `out`"""
        vals = _fr(vals)
        out = fr_empty(vals.shape[0])
        _chk(lib().kzg_hip_inplace_fft_fr(self.h, _p(vals), _p(out), vals.shape[0], int(inv)), error_ok=True)
        return out

    def fft_batch(self, vals, inv=False):
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        b, n = vals.shape[0], vals.shape[1]
        out = np.zeros_like(vals)
        _chk(lib().kzg_hip_fft_fr_batch(self.h, _p(vals), n, b, int(inv), _p(out)), error_ok=True)
        return out

    def fft_g1(self, vals, inv=False):
        """FFTSettings.FFTG1 (fft_g1.go:58-94)"""
        vals = _g1(vals)
        out = g1_empty(vals.shape[0])
        _chk(lib().kzg_hip_fft_g1(self.h, _p(vals), vals.shape[0], int(inv), _p(out)), error_ok=True)
        return out

    def fft_g1_batch(self, vals, inv=False):
        """FFTG1 on every row of vals (batch, n, 3, 6)"""
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        out = np.zeros_like(vals)
        _chk(lib().kzg_hip_fft_g1_batch(self.h, _p(vals), vals.shape[1], vals.shape[0], int(inv), _p(out)), error_ok=True)
        return out

    def evaluate_poly_in_evaluation_form(self, poly, x, scale=0):
        """bls.EvaluatePolyInEvaluationForm(y, poly, x, fs.ExpandedRootsOfUnity[:fs.MaxWidth], scale) (bls/globals.go:106-153)"""
        poly, x, y = _fr(poly), _fr(x), fr_empty(1)
        _chk(lib().kzg_hip_evaluate_poly_in_evaluation_form(self.h, _p(poly), poly.shape[0], _p(x), scale, _p(y)))
        return y[0]

    def das_fft_extension(self, vals):
        """FFTSettings.DASFFTExtension (das_extension.go:71-84); returns the odd values (the reference writes in place)"""
        vals = _fr(vals).copy()
        _chk(lib().kzg_hip_das_fft_extension(self.h, _p(vals), vals.shape[0]))
        return vals

    def das_fft_extension_batch(self, vals):
        vals = np.ascontiguousarray(vals, dtype=np.uint64).copy()
        _chk(lib().kzg_hip_das_fft_extension_batch(self.h, _p(vals), vals.shape[1], vals.shape[0]))
        return vals

    def fr_from_32(self, data):
        """bls.FrFrom32 over a slice (bls/bignum_kilic.go:33-44): (n, 32) LE bytes -> ((n, 4) images, all_ok)"""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, 32)
        out, ok = fr_empty(data.shape[0]), C.c_int(1)
        _chk(lib().kzg_hip_fr_from_le32(self.h, _p(data), data.shape[0], _p(out), C.byref(ok)))
        return out, bool(ok.value)

    def fr_to_32(self, vals):
        """bls.FrTo32 over a slice (bls/bignum_kilic.go:46-55)"""
        vals = _fr(vals)
        out = np.zeros((vals.shape[0], 32), dtype=np.uint8)
        _chk(lib().kzg_hip_fr_to_le32(self.h, _p(vals), vals.shape[0], _p(out)))
        return out

    def calibrate(self):
        """measured issue rates of this GPU: (v_mad_u64_u32 lane-ops/s, v_add_u32 lane-ops/s, lazy F_p products/s)"""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        _chk(lib().kzg_hip_calibrate(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def zero_poly_via_multiplication(self, missing_indices, length):
        """FFTSettings.ZeroPolyViaMultiplication (zero_poly.go:116-217): (zero_eval, zero_poly)"""
        mi = np.ascontiguousarray(missing_indices, dtype=np.uint64)
        ze, zp = fr_empty(length), fr_empty(length)
        _chk(lib().kzg_hip_zero_poly_via_multiplication(self.h, _p(mi), mi.shape[0], length, _p(ze), _p(zp)))
        return ze, zp

    def recover_poly_from_samples(self, samples, present):
        """FFTSettings.RecoverPolyFromSamples (recover_from_samples.go:42-109); present[i] False <=> samples[i] is nil"""
        samples = _fr(samples)
        present = np.ascontiguousarray(present, dtype=np.uint8)
        out = fr_empty(samples.shape[0])
        st = lib().kzg_hip_recover_poly_from_samples(self.h, _p(samples), _p(present), samples.shape[0], _p(out))
        if st == ERR_RECOVERY:
            raise KzgError(st, "failed to reconstruct data correctly")
        _chk(st, error_ok=True)
        return out

    def recover_poly_from_samples_batch(self, samples, present):
        """RecoverPolyFromSamples on every row of samples (batch, n, 4); present: (n,) one mask shared by every row, or (batch, n).  Returns (rows, status):
        status[b] is OK, ERR_RECOVERY or ERR_BAD_ARG (nothing present), a failed row is zero-filled, a row with nothing missing is copied through"""
        samples = np.ascontiguousarray(samples, dtype=np.uint64)
        present = np.ascontiguousarray(present, dtype=np.uint8)
        batch, n = samples.shape[0], samples.shape[1]
        if present.shape not in ((n,), (batch, n)):
            raise KzgPanic(ERR_LEN_MISMATCH, "present must have shape (n,) or (batch, n)")
        out, status = np.zeros_like(samples), np.zeros(batch, dtype=np.uint8)
        _chk(lib().kzg_hip_recover_poly_from_samples_batch(self.h, _p(samples), _p(present), 1 if present.ndim == 1 else batch, n, batch, _p(out), _p(status)), error_ok=True)
        return out, status

    def zero_poly_via_multiplication_batch(self, missing_lists, length):
        """ZeroPolyViaMultiplication of every erasure set of missing_lists: (zero_evals, zero_polys, status), rows of `length`; status[b] is OK or ERR_BAD_ARG"""
        lists = [np.ascontiguousarray(m, dtype=np.uint64).reshape(-1) for m in missing_lists]
        off = np.zeros(len(lists) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([m.shape[0] for m in lists], dtype=np.uint64)
        flat = np.concatenate(lists + [np.zeros(1, dtype=np.uint64)])      # (never empty: a pointer for a call whose sets are all empty)
        ze, zp, status = np.zeros((len(lists), length, 4), dtype=np.uint64), np.zeros((len(lists), length, 4), dtype=np.uint64), np.zeros(len(lists), dtype=np.uint8)
        _chk(lib().kzg_hip_zero_poly_via_multiplication_batch(self.h, _p(flat), _p(off), len(lists), length, _p(ze), _p(zp), _p(status)), error_ok=True)
        return ze, zp, status

    def bench_threads_fft(self, rows, threads, calls):
        """`threads` native host threads x `calls` blocking FFT calls on host buffers (kzg_hip_bench_threads_fft_fr): (calls per second, last results)"""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out, secs = np.zeros((threads, rows.shape[1], 4), dtype=np.uint64), C.c_double(0)
        _chk(lib().kzg_hip_bench_threads_fft_fr(self.h, _p(rows), rows.shape[1], rows.shape[0], threads, calls, _p(out), C.byref(secs)))
        return threads * calls / secs.value, out

    # ---- bls.* batch helpers that need a device context ----
    def lin_comb_g1(self, numbers, factors):
        """bls.LinCombG1 (bls/bls_kilic.go:132-150)"""
        numbers, factors = _g1(numbers), _fr(factors)
        if numbers.shape[0] != factors.shape[0]:
            raise KzgPanic(ERR_LEN_MISMATCH, "got LinCombG1 numbers/factors length mismatch")
        out = g1_empty(1)
        _chk(lib().kzg_hip_lincomb_g1(self.h, _p(numbers), _p(factors), numbers.shape[0], _p(out)))
        return out[0]

    def lincomb_promotions(self):
        """(point sets promoted so far, calls served by a promoted set): kzg_hip_lincomb_g1 turns a caller-supplied point set that keeps coming back into a cached one"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _chk(lib().kzg_hip_lincomb_promotions(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def to_compressed_g1(self, points):
        points = _g1(points)
        out = np.zeros((points.shape[0], 48), dtype=np.uint8)
        _chk(lib().kzg_hip_g1_to_compressed(self.h, _p(points), points.shape[0], _p(out)))
        return out

    def from_compressed_g1(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, 48)
        out = g1_empty(data.shape[0])
        _chk(lib().kzg_hip_g1_from_compressed(self.h, _p(data), data.shape[0], _p(out)))
        return out

    def g2_from_compressed(self, data):
        """bls.FromCompressedG2 over (n, 96) uint8 ZCash encodings -> (n, 3, 2, 6) Kilic G2 images; KzgPanic(ERR_BAD_POINT) if any is invalid"""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, 96)
        out = g2_empty(data.shape[0])
        _chk(lib().kzg_hip_g2_from_compressed(self.h, _p(data), data.shape[0], _p(out)))
        return out

    def pairings_verify_batch(self, a1, a2, b1, b2):
        """bls.PairingsVerify over rows: ok[i] = e(a1[i], a2[i]) == e(b1[i], b2[i])"""
        a1, b1, a2, b2 = _g1(a1), _g1(b1), _g2(a2), _g2(b2)
        n = a1.shape[0]
        if not (b1.shape[0] == a2.shape[0] == b2.shape[0] == n):
            raise KzgError(ERR_LEN_MISMATCH, "one point of each kind per check")
        ok = np.zeros(n, dtype=np.uint8)
        _chk(lib().kzg_hip_pairings_verify_batch(self.h, _p(a1), _p(a2), _p(b1), _p(b2), n, _p(ok)))
        return ok.astype(bool)

    def pairing_test(self, g1, g2):
        """test hook: e(g1[i], g2[i])^(3 (p^12 - 1) / r) as 12 standard-form F_p integers per pair (memory order of the tower)"""
        g1, g2 = _g1(g1), _g2(g2)
        n = g1.shape[0]
        out = np.zeros((n, 12, 6), dtype=np.uint64)
        _chk(lib().kzg_hip_pairing_test(self.h, _p(g1), _p(g2), n, _p(out)))
        return [[sum(int(v[k][i]) << (64 * i) for i in range(6)) for k in range(12)] for v in out]

    def pairing_test_wave(self, g1, g2):
        """test hook: pairing_test on the kernel with one wavefront per pair"""
        g1, g2 = _g1(g1), _g2(g2)
        n = g1.shape[0]
        out = np.zeros((n, 12, 6), dtype=np.uint64)
        _chk(lib().kzg_hip_pairing_test_wave(self.h, _p(g1), _p(g2), n, _p(out)))
        return [[sum(int(v[k][i]) << (64 * i) for i in range(6)) for k in range(12)] for v in out]

    def wave_fp12_op(self, op, a, b):
        """test hook: one tower operation per row on the wavefront tower; a, b: (n, 144) uint32 rows of 12 standard-form F_p elements"""
        a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
        assert a.shape == b.shape and a.ndim == 2 and a.shape[1] == 144
        out = np.zeros_like(a)
        _chk(lib().kzg_hip_test_wave_fp12_op(self.h, op, _p(a), _p(b), a.shape[0], _p(out)))
        return out

    def g1_marshal_text(self, points):
        """bls.G1Point.MarshalText over a slice (bls/bls_all.go:20-22): lower-case hex of the 48-byte compressed form"""
        points = _g1(points)
        n = points.shape[0]
        buf = C.create_string_buffer(96 * n + 1)
        _chk(lib().kzg_hip_g1_marshal_text(self.h, _p(points), n, buf))
        txt = buf.raw[:96 * n].decode("ascii")
        return [txt[96 * i:96 * i + 96] for i in range(n)]

    def g1_unmarshal_text(self, texts):
        """bls.G1Point.UnmarshalText over a slice (bls/bls_all.go:24-39); hex decoding in the library, decompression on the device"""
        texts = list(texts)
        if any(len(t) != 96 for t in texts):
            raise KzgPanic(ERR_BAD_POINT, "expected 48-byte compressed G1 points")
        out = g1_empty(len(texts))
        _chk(lib().kzg_hip_g1_unmarshal_text(self.h, "".join(texts).encode("ascii", "replace"), len(texts), _p(out)))
        return out

    def trusted_setup_from_json(self, text):
        """JSONTrustedSetup (eth/globals.go:33-49): JSON text -> (setup_G1, setup_G1_lagrange) as Kilic images; trusted_setup_g2_from_json reads setup_G2"""
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        n1, n2 = C.c_uint64(0), C.c_uint64(0)
        _chk(lib().kzg_hip_trusted_setup_from_json(self.h, raw, len(raw), None, None, 0, C.byref(n1), C.byref(n2)))
        cap = max(n1.value, n2.value, 1)
        mono, lag = g1_empty(cap), g1_empty(cap)
        _chk(lib().kzg_hip_trusted_setup_from_json(self.h, raw, len(raw), _p(mono), _p(lag), cap, C.byref(n1), C.byref(n2)))
        return mono[:n1.value], lag[:n2.value]

    def mul_g1_vec(self, points, scalars):
        points, scalars = _g1(points), _fr(scalars)
        out = g1_empty(points.shape[0])
        _chk(lib().kzg_hip_g1_mul_vec(self.h, _p(points), _p(scalars), points.shape[0], _p(out)))
        return out

    def generate_testing_setup_g1(self, secret_fr, n):
        """GenerateTestingSetup (setup.go:9-26), G1 half; secret_fr is the Montgomery image of the secret"""
        secret_fr = _fr(secret_fr)
        out = g1_empty(n)
        _chk(lib().kzg_hip_generate_testing_setup_g1(self.h, _p(secret_fr), n, _p(out)))
        return out


    def mul_gen_g2_vec(self, scalars):
        """bls.MulG2(&out[i], &bls.GenG2, &scalars[i]) over a slice -> (n, 3, 2, 6) Kilic G2 images with Z = 1 (infinity: (0, 1, 0))"""
        scalars = _fr(scalars)
        out = g2_empty(scalars.shape[0])
        _chk(lib().kzg_hip_g2_mul_generator_vec(self.h, _p(scalars), scalars.shape[0], _p(out)))
        return out

    def generate_testing_setup_g2(self, secret_fr, n):
        """GenerateTestingSetup (setup.go:9-26), G2 half: out[i] = [secret^i] G2; secret_fr is the Montgomery image of the secret"""
        secret_fr = _fr(secret_fr)
        out = g2_empty(n)
        _chk(lib().kzg_hip_generate_testing_setup_g2(self.h, _p(secret_fr), n, _p(out)))
        return out

    def to_compressed_g2(self, points):
        """bls.ToCompressedG2 over a slice (bls/bls_kilic.go:123-125): (n, 3, 2, 6) images, any Z -> (n, 96) uint8"""
        points = _g2(points)
        out = np.zeros((points.shape[0], 96), dtype=np.uint8)
        _chk(lib().kzg_hip_g2_to_compressed(self.h, _p(points), points.shape[0], _p(out)))
        return out

    def g2_marshal_text(self, points):
        """bls.G2Point.MarshalText over a slice (bls/bls_all.go:41-43): lower-case hex of the 96-byte compressed form"""
        return [bytes(row).hex() for row in self.to_compressed_g2(points)]

    def g2_unmarshal_text(self, texts):
        """bls.G2Point.UnmarshalText over a slice (bls/bls_all.go:45-60): hex decoding here, decompression and subgroup check on the device"""
        texts = list(texts)
        try:
            raw = [bytes.fromhex(t) for t in texts]
        except ValueError:
            raise KzgPanic(ERR_BAD_POINT, "invalid hex in a G2 point") from None
        if any(len(r) != 96 for r in raw):
            raise KzgPanic(ERR_BAD_POINT, "expected 96-byte compressed G2 points")
        return self.g2_from_compressed(np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(-1, 96))

    def trusted_setup_g2_from_json(self, text):
        """the "setup_G2" array of a JSONTrustedSetup document (eth/globals.go:35,47) as Kilic G2 images; none when the key is absent"""
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        n = C.c_uint64(0)
        _chk(lib().kzg_hip_trusted_setup_g2_from_json(self.h, raw, len(raw), None, 0, C.byref(n)))
        out = g2_empty(n.value)
        if n.value:
            _chk(lib().kzg_hip_trusted_setup_g2_from_json(self.h, raw, len(raw), _p(out), n.value, C.byref(n)))
        return out[:n.value]

    def g2_table_builds(self):
        """test hook: how many times this handle built its fixed-base table of bls.GenG2"""
        n = C.c_uint64(0)
        _chk(lib().kzg_hip_test_g2_table_builds(self.h, C.byref(n)))
        return n.value


def generate_testing_setup(fs, secret_fr, n):
    """GenerateTestingSetup (setup.go:9-26): ([secret^i] G1, [secret^i] G2) for i < n, both halves on the device"""
    return fs.generate_testing_setup_g1(secret_fr, n), fs.generate_testing_setup_g2(secret_fr, n)


class G1Points:
    """a point set kept in HBM for repeated bls.LinCombG1 calls (kzg_hip_points_*): CommitToEvalPoly's secretG1IFFT, eth's Lagrange setup"""

    def __init__(self, fs, points):
        points = _g1(points)
        h = C.c_void_p()
        _chk(lib().kzg_hip_points_new(fs.h, _p(points), points.shape[0], C.byref(h)))
        self.h, self.fs, self.n = h, fs, points.shape[0]

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_points_free(self.h)
            self.h = None

    def set_table_budget_gb(self, gb):
        """HBM budget of the set's fixed-base table (0: bucket pipeline only); see kzg_hip_points_set_table_budget_gb"""
        _chk(lib().kzg_hip_points_set_table_budget_gb(self.h, float(gb)))

    def lin_comb(self, factors):
        """bls.LinCombG1(points[:len(factors)], factors)"""
        factors = _fr(factors)
        out = g1_empty(1)
        _chk(lib().kzg_hip_lincomb_points(self.h, _p(factors), factors.shape[0], _p(out)))
        return out[0]

    def lin_comb_batch(self, factors):
        factors = np.ascontiguousarray(factors, dtype=np.uint64)
        b, n = factors.shape[0], factors.shape[1]
        out = g1_empty(b)
        _chk(lib().kzg_hip_lincomb_points_batch(self.h, _p(factors), n, b, _p(out)))
        return out


def commit_to_eval_poly(fs, secret_g1_ifft, eval_poly):
    """kzg.CommitToEvalPoly (kzg_single_proofs.go:12-14)"""
    return fs.lin_comb_g1(secret_g1_ifft, eval_poly)


class KZGSettings:
    """kzg.KZGSettings (kzg.go:11-36): SecretG1 is uploaded once and stays in HBM; with secret_g2 the object also verifies (set_secret_g2)."""

    def __init__(self, fs, secret_g1, secret_g2=None):
        secret_g1 = _g1(secret_g1)
        if secret_g2 is not None:
            secret_g2 = _g2(secret_g2)
            if secret_g2.shape[0] != secret_g1.shape[0]:
                raise KzgPanic(ERR_LEN_MISMATCH, "secret list lengths don't match")   # kzg.go:22-27
        h = C.c_void_p()
        _chk(lib().kzg_hip_kzg_settings_new(fs.h, _p(secret_g1), secret_g1.shape[0], C.byref(h)))
        self.h, self.fs, self.n_setup = h, fs, secret_g1.shape[0]
        if secret_g2 is not None:
            try:
                self.set_secret_g2(secret_g2)
            except KzgError:
                self.close()
                raise

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_kzg_settings_free(self.h)
            self.h = None

    def commit_to_poly_unoptimized(self, coeffs):
        """KZGSettings.CommitToPolyUnoptimized (kzg_single_proofs.go:22-33): the same group element as CommitToPoly, hence the same call"""
        return self.commit_to_poly(coeffs)

    def set_table_budget_gb(self, gb):
        """HBM budget of the fixed-base commitment table (default 110 GB: 4096 points get signed 16-bit windows, 8 of them walked by both GLV halves, 103 GB)"""
        _chk(lib().kzg_hip_kzg_set_table_budget_gb(self.h, float(gb)))

    def bench_drop_in(self, blobs, threads, calls, op=0):
        """`threads` native host threads x `calls` blocking one-polynomial calls (kzg_hip_bench_drop_in): (calls per second, last results)"""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint64)
        out, secs = g1_empty(threads), C.c_double(0)
        _chk(lib().kzg_hip_bench_drop_in(self.h, op, _p(blobs), blobs.shape[1], blobs.shape[0], threads, calls, _p(out), C.byref(secs)))
        return threads * calls / secs.value, out

    def coalesce_stats(self, op=0):
        """cumulative statistics of the coalescer behind the one-polynomial calls (op 0 CommitToPoly, 1 ComputeProofSingle)"""
        a = (C.c_uint64 * 8)()
        _chk(lib().kzg_hip_coalesce_stats(self.h, op, a))
        req, bat = a[0], a[1]
        return {"requests": req, "batches": bat, "avg_batch": req / bat if bat else 0.0,
                "ms_per_batch": {"executing": a[2] * 1e-6 / bat if bat else 0.0, "waiting_for_a_device_slot": a[3] * 1e-6 / bat if bat else 0.0,
                                 "gathering_callers": a[4] * 1e-6 / bat if bat else 0.0, "waiting_for_row_copies": a[5] * 1e-6 / bat if bat else 0.0},
                "largest_concurrency_estimate": a[6], "batches_in_flight_limit": a[7]}

    def table_info(self):
        """(window bits, windows, bytes) of the fixed-base table the commitments walk; zeros before the first commitment"""
        c, w, b = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        _chk(lib().kzg_hip_kzg_table_info(self.h, C.byref(c), C.byref(w), C.byref(b)))
        return c.value, w.value, b.value

    def set_projective_outputs(self, on=True):
        """CommitToPoly / ComputeProofSingle return un-normalised Jacobian images (the reference's own return type): no inversion per result"""
        _chk(lib().kzg_hip_kzg_set_projective_outputs(self.h, 1 if on else 0))

    def table_additions(self):
        """mixed additions per coefficient on that table (2 x windows: both GLV halves of a scalar walk the same rows)"""
        return lib().kzg_hip_kzg_table_additions(self.h)

    def commit_to_poly(self, coeffs):
        coeffs = _fr(coeffs)
        out = g1_empty(1)
        _chk(lib().kzg_hip_commit_to_poly(self.h, _p(coeffs), coeffs.shape[0], _p(out)))
        return out[0]

    def commit_to_poly_batch(self, coeffs):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
        b, n = coeffs.shape[0], coeffs.shape[1]
        out = g1_empty(b)
        _chk(lib().kzg_hip_commit_to_poly_batch(self.h, _p(coeffs), n, b, _p(out)))
        return out

    def compute_proof_single(self, poly, x):
        poly = _fr(poly)
        out = g1_empty(1)
        _chk(lib().kzg_hip_compute_proof_single(self.h, _p(poly), poly.shape[0], x, _p(out)))
        return out[0]

    def compute_proof_single_batch(self, polys, xs):
        """ComputeProofSingle on a batch: polys (batch, n, 4), xs (batch,) uint64 -> (batch, 3, 6)"""
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        b, n = polys.shape[0], polys.shape[1]
        out = g1_empty(b)
        _chk(lib().kzg_hip_compute_proof_single_batch(self.h, _p(polys), n, b, _p(xs), _p(out)))
        return out

    def compute_proof_multi(self, poly, x, n):
        """KZGSettings.ComputeProofMulti (kzg_multi_proofs.go:13-43), reference quirk (divisor X^n) included"""
        poly = _fr(poly)
        out = g1_empty(1)
        _chk(lib().kzg_hip_compute_proof_multi(self.h, _p(poly), poly.shape[0], x, n, _p(out)))
        return out[0]

    def check_proof_multi_interpolation(self, ys, x):
        """prover-side half of KZGSettings.CheckProofMulti (kzg_multi_proofs.go:47-75): ([I(s)]_1, x^n)"""
        ys, x = _fr(ys), _fr(x)
        out, xp = g1_empty(1), fr_empty(1)
        _chk(lib().kzg_hip_check_proof_multi_interpolation(self.h, _p(ys), ys.shape[0], _p(x), _p(out), _p(xp)))
        return out[0], xp[0]

    def set_secret_g2(self, secret_g2):
        """KZGSettings.SecretG2 (kzg.go:11-19): (n, 3, 2, 6) G2 images, n >= 2"""
        g2 = _g2(secret_g2)
        _chk(lib().kzg_hip_kzg_set_secret_g2(self.h, _p(g2), g2.shape[0]))

    def check_proof_single_batch(self, commitments, proofs, xs, ys):
        """KZGSettings.CheckProofSingle (kzg_single_proofs.go:57-70) over rows -> bool mask"""
        c, pi, xs, ys = _g1(commitments), _g1(proofs), _fr(xs), _fr(ys)
        n = c.shape[0]
        if not (pi.shape[0] == xs.shape[0] == ys.shape[0] == n):
            raise KzgError(ERR_LEN_MISMATCH, "one commitment, proof, x and y per check")
        ok = np.zeros(n, dtype=np.uint8)
        _chk(lib().kzg_hip_check_proof_single_batch(self.h, _p(c), _p(pi), _p(xs), _p(ys), n, _p(ok)))
        return ok.astype(bool)

    def check_proof_single_batch_combined(self, commitments, proofs, xs, ys, seed=None):
        """the same mask with one pairing check per group of rows (kzg_hip_check_proof_single_batch_combined): a random linear combination per
        group, the rows of a failing group re-checked one by one.  seed: 32 bytes for reproducible runs, None: drawn from the operating system
        (a seed the prover can know in advance voids the 2^-128 bound).  Presupposes points of G1, as CheckProofSingle does"""
        c, pi, xs, ys = _g1(commitments), _g1(proofs), _fr(xs), _fr(ys)
        n = c.shape[0]
        if not (pi.shape[0] == xs.shape[0] == ys.shape[0] == n):
            raise KzgError(ERR_LEN_MISMATCH, "one commitment, proof, x and y per check")
        ok = np.zeros(n, dtype=np.uint8)
        _chk(lib().kzg_hip_check_proof_single_batch_combined(self.h, _p(c), _p(pi), _p(xs), _p(ys), n, _seed32(seed), _p(ok)))
        return ok.astype(bool)

    def test_combine_points(self, commitments, proofs, xs, ys, seed):
        """test hook: (A_g, B_g) of every group of the combined check for these inputs and this seed, normalised images"""
        c, pi, xs, ys = _g1(commitments), _g1(proofs), _fr(xs), _fr(ys)
        n = c.shape[0]
        groups = -(-n // combine_stats()["rows"])
        a, b = g1_empty(groups), g1_empty(groups)
        _chk(lib().kzg_hip_test_combine_points(self.h, _p(c), _p(pi), _p(xs), _p(ys), n, _seed32(seed), _p(a), _p(b)))
        return a, b

    def check_proof_multi_batch(self, commitments, proofs, xs, ys):
        """KZGSettings.CheckProofMulti (kzg_multi_proofs.go:47-75) over rows; ys is (count, n, 4) -> bool mask"""
        c, pi, xs = _g1(commitments), _g1(proofs), _fr(xs)
        count = c.shape[0]
        ys = np.ascontiguousarray(ys, dtype=np.uint64)
        ys = ys if ys.ndim == 3 else ys.reshape(count, -1, 4)
        if ys.shape[0] != count or ys.shape[2] != 4:
            raise KzgError(ERR_LEN_MISMATCH, "one row of ys per check")
        if not (pi.shape[0] == xs.shape[0] == count):
            raise KzgError(ERR_LEN_MISMATCH, "one commitment, proof and x per check")
        ok = np.zeros(count, dtype=np.uint8)
        _chk(lib().kzg_hip_check_proof_multi_batch(self.h, _p(c), _p(pi), _p(xs), _p(ys), ys.shape[1], count, _p(ok)))
        return ok.astype(bool)

    def _multi_rows(self, commitments, proofs, xs, ys):
        c, pi, xs = _g1(commitments), _g1(proofs), _fr(xs)
        count = c.shape[0]
        ys = np.ascontiguousarray(ys, dtype=np.uint64)
        ys = ys if ys.ndim == 3 else ys.reshape(count, -1, 4)
        if ys.shape[0] != count or ys.shape[2] != 4:
            raise KzgError(ERR_LEN_MISMATCH, "one row of ys per check")
        if not (pi.shape[0] == xs.shape[0] == count):
            raise KzgError(ERR_LEN_MISMATCH, "one commitment, proof and x per check")
        return c, pi, xs, ys, count

    def check_proof_multi_batch_combined(self, commitments, proofs, xs, ys, seed=None):
        """the same mask with one pairing check per group of rows (kzg_hip_check_proof_multi_batch_combined): what a DAS sampler runs on coset
        proofs.  The rows of a failing group are re-checked one by one; no commitment table is built.  seed as check_proof_single_batch_combined.
        Presupposes points of G1, as CheckProofMulti does"""
        c, pi, xs, ys, count = self._multi_rows(commitments, proofs, xs, ys)
        ok = np.zeros(count, dtype=np.uint8)
        _chk(lib().kzg_hip_check_proof_multi_batch_combined(self.h, _p(c), _p(pi), _p(xs), _p(ys), ys.shape[1], count, _seed32(seed), _p(ok)))
        return ok.astype(bool)

    def test_combine_multi_points(self, commitments, proofs, xs, ys, seed):
        """test hook: (A_g, B_g, J_g) of every group of the combined multi check for these inputs and this seed: normalised images, and
        (groups, np, 4) Montgomery values"""
        c, pi, xs, ys, count = self._multi_rows(commitments, proofs, xs, ys)
        groups = -(-count // combine_stats()["rows"])
        n = ys.shape[1]
        npad = 1 if n <= 1 else 1 << (n - 1).bit_length()
        a, b, j = g1_empty(groups), g1_empty(groups), np.zeros((groups, npad, 4), dtype=np.uint64)
        _chk(lib().kzg_hip_test_combine_multi_points(self.h, _p(c), _p(pi), _p(xs), _p(ys), n, count, _seed32(seed), _p(a), _p(b), _p(j)))
        return a, b, j

    def toeplitz_part2(self, toeplitz_coeffs, x_ext_fft):
        toeplitz_coeffs, x_ext_fft = _fr(toeplitz_coeffs), _g1(x_ext_fft)
        if toeplitz_coeffs.shape[0] != x_ext_fft.shape[0]:
            raise KzgPanic(ERR_LEN_MISMATCH, "expected toeplitz coeffs to match xExtFFT length")
        out = g1_empty(x_ext_fft.shape[0])
        _chk(lib().kzg_hip_toeplitz_part2(self.h, _p(toeplitz_coeffs), _p(x_ext_fft), x_ext_fft.shape[0], _p(out)))
        return out

    def toeplitz_part3(self, h_ext_fft):
        h_ext_fft = _g1(h_ext_fft)
        out = g1_empty(h_ext_fft.shape[0] // 2)
        _chk(lib().kzg_hip_toeplitz_part3(self.h, _p(h_ext_fft), h_ext_fft.shape[0], _p(out)))
        return out


class FK20SingleSettings:
    """kzg.FK20SingleSettings (kzg.go:38-64; fk20_single.go:122-196)"""

    def __init__(self, ks, n2):
        h = C.c_void_p()
        _chk(lib().kzg_hip_fk20_single_settings_new(ks.h, n2, C.byref(h)))
        self.h, self.ks, self.n2 = h, ks, n2

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_fk20_single_settings_free(self.h)
            self.h = None

    def x_ext_fft(self):
        out = g1_empty(self.n2)
        _chk(lib().kzg_hip_fk20_single_x_ext_fft(self.h, _p(out)))
        return out

    def fk20_single(self, poly):
        poly = _fr(poly)
        out = g1_empty(poly.shape[0])
        _chk(lib().kzg_hip_fk20_single(self.h, _p(poly), poly.shape[0], _p(out)))
        return out

    def fk20_single_batch(self, polys):
        """FK20Single on each row of polys (batch, n, 4) -> (batch, n, 3, 6)"""
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        b, n = polys.shape[0], polys.shape[1]
        out = np.zeros((b, n, 3, 6), dtype=np.uint64)
        _chk(lib().kzg_hip_fk20_single_batch(self.h, _p(polys), n, b, _p(out)))
        return out

    def fk20_single_da_optimized(self, poly):
        poly = _fr(poly)
        out = g1_empty(poly.shape[0])
        _chk(lib().kzg_hip_fk20_single_da_optimized(self.h, _p(poly), poly.shape[0], _p(out)))
        return out

    def da_using_fk20(self, poly):
        poly = _fr(poly)
        out = g1_empty(2 * poly.shape[0])
        _chk(lib().kzg_hip_da_using_fk20(self.h, _p(poly), poly.shape[0], _p(out)))
        return out

    def da_using_fk20_batch(self, polys):
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        b, n = polys.shape[0], polys.shape[1]
        out = np.zeros((b, 2 * n, 3, 6), dtype=np.uint64)
        _chk(lib().kzg_hip_da_using_fk20_batch(self.h, _p(polys), n, b, _p(out)))
        return out


class FK20MultiSettings:
    """kzg.FK20MultiSettings (kzg.go:66-116; fk20_multi.go:25-133)"""

    def __init__(self, ks, n2, chunk_len):
        h = C.c_void_p()
        _chk(lib().kzg_hip_fk20_multi_settings_new(ks.h, n2, chunk_len, C.byref(h)))
        self.h, self.ks, self.n2, self.chunk_len = h, ks, n2, chunk_len

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_fk20_multi_settings_free(self.h)
            self.h = None

    def fk20_multi(self, poly):
        poly = _fr(poly)
        out = g1_empty(poly.shape[0] // self.chunk_len)
        _chk(lib().kzg_hip_fk20_multi(self.h, _p(poly), poly.shape[0], _p(out)))
        return out

    def fk20_multi_da_optimized(self, poly):
        poly = _fr(poly)
        out = g1_empty(poly.shape[0] // self.chunk_len)
        _chk(lib().kzg_hip_fk20_multi_da_optimized(self.h, _p(poly), poly.shape[0], _p(out)))
        return out

    def da_using_fk20_multi(self, poly):
        poly = _fr(poly)
        out = g1_empty(2 * poly.shape[0] // self.chunk_len)
        _chk(lib().kzg_hip_da_using_fk20_multi(self.h, _p(poly), poly.shape[0], _p(out)))
        return out

    def da_using_fk20_multi_batch(self, polys):
        """DAUsingFK20Multi on each row of polys (batch, n, 4) -> (batch, 2n / chunk_len, 3, 6)"""
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        b, n = polys.shape[0], polys.shape[1]
        out = np.zeros((b, 2 * n // self.chunk_len, 3, 6), dtype=np.uint64)
        _chk(lib().kzg_hip_da_using_fk20_multi_batch(self.h, _p(polys), n, b, _p(out)))
        return out


class _Borrowed:
    """a settings object owned by a MultiKZGSettings: same methods, close() is a no-op"""

    def close(self):
        self.h = None


class _BorrowedFFT(_Borrowed, FFTSettings):
    def __init__(self, h, max_scale, device):
        self.h, self.max_scale, self.max_width, self.device = C.c_void_p(h), max_scale, 1 << max_scale, device


class _BorrowedKZG(_Borrowed, KZGSettings):
    def __init__(self, h, fs, n_setup):
        self.h, self.fs, self.n_setup = C.c_void_p(h), fs, n_setup


class MultiKZGSettings:
    """NewFFTSettings(max_scale) + NewKZGSettings(fs, secret_g1) on EVERY device of `devices`, behind one handle
    (kzg_hip_multi_*, include/kzg_hip.h): what the Go shim exposes as kzg.NewMultiKZGSettings.  A list may repeat a device."""

    def __init__(self, devices, max_scale, secret_g1):
        secret_g1 = _g1(secret_g1)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _chk(lib().kzg_hip_multi_settings_new(devs, len(devices), max_scale, _p(secret_g1), secret_g1.shape[0], C.byref(h)))
        self.h, self.devices, self.max_scale, self.n_setup = h, list(devices), max_scale, secret_g1.shape[0]

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_multi_settings_free(self.h)
            self.h = None

    @property
    def transport(self):
        """"rccl" (ncclAllGather between distinct devices), "peer-copy" (hipMemcpyPeerAsync: a repeated device, or no librccl) or
        "host-staged" (device -> pinned host -> device: what is left when the other two fail the creation-time self-test)"""
        return lib().kzg_hip_multi_transport(self.h).decode()

    @property
    def transport_self_test(self):
        """outcome of the exchange test the constructor ran: "ok: <transport>, <entries> entries, ..." """
        return lib().kzg_hip_multi_transport_check(self.h).decode()

    @property
    def transport_note(self):
        return lib().kzg_hip_multi_transport_note(self.h).decode()

    @property
    def exchanges(self):
        return lib().kzg_hip_multi_exchanges(self.h)

    def fft_settings(self, i):
        return _BorrowedFFT(lib().kzg_hip_multi_fft(self.h, i), self.max_scale, lib().kzg_hip_multi_device(self.h, i))

    def kzg_settings(self, i):
        """entry i's KZGSettings (borrowed): every single-device method on a chosen device"""
        return _BorrowedKZG(lib().kzg_hip_multi_kzg(self.h, i), self.fft_settings(i), self.n_setup)

    def set_fft_sharding(self, mode):
        """one-polynomial FK20 calls: "gather" (all-gather of hExtFFT, transforms on the first device), "sharded" (both G1 transforms
        sharded too: five all-gathers) or None (default: sharded from 4 devices on)"""
        _chk(lib().kzg_hip_multi_set_fft_sharding(self.h, {None: -1, "gather": 0, "sharded": 1}[mode]))

    def set_table_budget_gb(self, gb):
        _chk(lib().kzg_hip_multi_set_table_budget_gb(self.h, float(gb)))

    def commit_to_poly_batch(self, coeffs):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
        b, n = coeffs.shape[0], coeffs.shape[1]
        out = g1_empty(b)
        _chk(lib().kzg_hip_multi_commit_to_poly_batch(self.h, _p(coeffs), n, b, _p(out)))
        return out

    def fft_batch(self, vals, inv=False):
        """FFT (fft_fr.go:55-74) on every row, rows divided among the devices"""
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        out = np.zeros_like(vals)
        _chk(lib().kzg_hip_multi_fft_fr_batch(self.h, _p(vals), vals.shape[1], vals.shape[0], int(inv), _p(out)), error_ok=True)
        return out

    def fft_g1_batch(self, vals, inv=False):
        """FFTG1 (fft_g1.go:58-94) on every row, rows divided among the devices"""
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        out = np.zeros_like(vals)
        _chk(lib().kzg_hip_multi_fft_g1_batch(self.h, _p(vals), vals.shape[1], vals.shape[0], int(inv), _p(out)), error_ok=True)
        return out

    def das_fft_extension_batch(self, vals):
        """DASFFTExtension (das_extension.go:71-84) on every row; returns the odd values"""
        vals = np.ascontiguousarray(vals, dtype=np.uint64).copy()
        _chk(lib().kzg_hip_multi_das_fft_extension_batch(self.h, _p(vals), vals.shape[1], vals.shape[0]))
        return vals

    def compute_proof_single_batch(self, polys, xs):
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        b, n = polys.shape[0], polys.shape[1]
        out = g1_empty(b)
        _chk(lib().kzg_hip_multi_compute_proof_single_batch(self.h, _p(polys), n, b, _p(xs), _p(out)))
        return out


class MultiEthSettings:
    """package eth (eth/globals.go:39-72) on every device of a MultiKZGSettings: batches divided among the devices"""

    def __init__(self, mks, setup_g1_lagrange):
        lag = _g1(setup_g1_lagrange)
        h = C.c_void_p()
        _chk(lib().kzg_hip_multi_eth_settings_new(mks.h, _p(lag), lag.shape[0], C.byref(h)))
        self.h, self.mks, self.n = h, mks, lag.shape[0]

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_multi_eth_settings_free(self.h)
            self.h = None

    def blob_to_kzg_commitment_batch(self, blobs):
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.n, 32)
        b = blobs.shape[0]
        out, ok = np.zeros((b, 48), dtype=np.uint8), np.zeros(b, dtype=np.uint8)
        _chk(lib().kzg_hip_multi_eth_blob_to_kzg_commitment_batch(self.h, _p(blobs), b, _p(out), _p(ok)))
        return out, ok.astype(bool)

    def compute_kzg_proof_batch(self, polynomials, zs):
        polys = np.ascontiguousarray(polynomials, dtype=np.uint64).reshape(-1, self.n, 4)
        zs = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4)
        b = polys.shape[0]
        if zs.shape[0] != b:
            raise KzgError(ERR_LEN_MISMATCH, "one z per polynomial")
        out, ys, ok = np.zeros((b, 48), dtype=np.uint8), fr_empty(b), np.zeros(b, dtype=np.uint8)
        _chk(lib().kzg_hip_multi_eth_compute_kzg_proof_batch(self.h, _p(polys), self.n, b, _p(zs), _p(out), _p(ys), _p(ok)))
        return out, ys, ok.astype(bool)


class MultiFK20SingleSettings:
    """NewFK20SingleSettings (kzg.go:43-64) on every device of a MultiKZGSettings"""

    def __init__(self, mks, n2):
        h = C.c_void_p()
        _chk(lib().kzg_hip_multi_fk20_single_settings_new(mks.h, n2, C.byref(h)))
        self.h, self.mks, self.n2 = h, mks, n2

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_multi_fk20_single_settings_free(self.h)
            self.h = None

    def da_using_fk20(self, poly):
        """ONE polynomial over all devices (Toeplitz stage by output position + all-gather(s))"""
        poly = _fr(poly)
        out = g1_empty(2 * poly.shape[0])
        _chk(lib().kzg_hip_multi_da_using_fk20(self.h, _p(poly), poly.shape[0], _p(out)), error_ok=True)
        return out

    def da_using_fk20_batch(self, polys):
        """polynomials divided among the devices"""
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        b, n = polys.shape[0], polys.shape[1]
        out = np.zeros((b, 2 * n, 3, 6), dtype=np.uint64)
        _chk(lib().kzg_hip_multi_da_using_fk20_batch(self.h, _p(polys), n, b, _p(out)))
        return out


class MultiFK20MultiSettings:
    """NewFK20MultiSettings (kzg.go:73-116) on every device of a MultiKZGSettings"""

    def __init__(self, mks, n2, chunk_len):
        h = C.c_void_p()
        _chk(lib().kzg_hip_multi_fk20_multi_settings_new(mks.h, n2, chunk_len, C.byref(h)))
        self.h, self.mks, self.n2, self.chunk_len = h, mks, n2, chunk_len

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_multi_fk20_multi_settings_free(self.h)
            self.h = None

    def da_using_fk20_multi(self, poly):
        """ONE polynomial over all devices (fk20_multi.go:113-133)"""
        poly = _fr(poly)
        out = g1_empty(2 * poly.shape[0] // self.chunk_len)
        _chk(lib().kzg_hip_multi_da_using_fk20_multi(self.h, _p(poly), poly.shape[0], _p(out)), error_ok=True)
        return out

    def da_using_fk20_multi_batch(self, polys):
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        b, n = polys.shape[0], polys.shape[1]
        out = np.zeros((b, 2 * n // self.chunk_len, 3, 6), dtype=np.uint64)
        _chk(lib().kzg_hip_multi_da_using_fk20_multi_batch(self.h, _p(polys), n, b, _p(out)))
        return out


class EthSettings:
    """eth/ package state (eth/globals.go:39-72): bit-reversed Lagrange setup + bit-reversed domain, device resident."""

    def __init__(self, fs, setup_g1_lagrange):
        lag = _g1(setup_g1_lagrange)
        h = C.c_void_p()
        _chk(lib().kzg_hip_eth_settings_new(fs.h, _p(lag), lag.shape[0], C.byref(h)))
        self.h, self.fs, self.n = h, fs, lag.shape[0]

    def close(self):
        if getattr(self, "h", None):
            lib().kzg_hip_eth_settings_free(self.h)
            self.h = None

    def blob_to_kzg_commitment_batch(self, blobs):
        """eth.BlobToKZGCommitment (eth/eth.go:145-151) on (batch, n, 32) uint8 little-endian blobs -> ((batch, 48) uint8, ok flags)"""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.n, 32)
        b = blobs.shape[0]
        out, ok = np.zeros((b, 48), dtype=np.uint8), np.zeros(b, dtype=np.uint8)
        _chk(lib().kzg_hip_eth_blob_to_kzg_commitment_batch(self.h, _p(blobs), b, _p(out), _p(ok)))
        return out, ok.astype(bool)

    def blob_to_kzg_commitment(self, blob):
        out, ok = self.blob_to_kzg_commitment_batch(np.asarray(blob, dtype=np.uint8).reshape(1, self.n, 32))
        return out[0], bool(ok[0])

    def compute_kzg_proof(self, polynomial, z):
        """eth.ComputeKZGProof (eth/helpers.go:179-203): returns (proof48, y); raises KzgError like the reference's errors"""
        poly, z = _fr(polynomial), _fr(z)
        out, y = np.zeros(48, dtype=np.uint8), fr_empty(1)
        st = lib().kzg_hip_eth_compute_kzg_proof(self.h, _p(poly), poly.shape[0], _p(z), _p(out), _p(y))
        if st == ERR_LEN_MISMATCH:
            raise KzgError(st, "polynomial has invalid length")
        if st == ERR_BAD_ARG:
            raise KzgError(st, "invalid z challenge")
        _chk(st)
        return out, y[0]

    def compute_kzg_proof_batch(self, polynomials, zs):
        """eth.ComputeKZGProof over rows (kzg_hip_eth_compute_kzg_proof_batch): ((batch, 48) uint8 proofs, (batch, 4) ys, ok flags); ok[b] is False
        where zs[b] lies in the domain (the reference's "invalid z challenge")"""
        polys = np.ascontiguousarray(polynomials, dtype=np.uint64).reshape(-1, self.n, 4)
        zs = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4)
        b = polys.shape[0]
        if zs.shape[0] != b:
            raise KzgError(ERR_LEN_MISMATCH, "one z per polynomial")
        out, ys, ok = np.zeros((b, 48), dtype=np.uint8), fr_empty(b), np.zeros(b, dtype=np.uint8)
        _chk(lib().kzg_hip_eth_compute_kzg_proof_batch(self.h, _p(polys), self.n, b, _p(zs), _p(out), _p(ys), _p(ok)))
        return out, ys, ok.astype(bool)

    def set_setup_g2(self, setup_g2):
        """kzgSetupG2 (eth/globals.go:47): (n, 3, 2, 6) G2 images, n >= 2"""
        g2 = _g2(setup_g2)
        _chk(lib().kzg_hip_eth_set_setup_g2(self.h, _p(g2), g2.shape[0]))

    def verify_kzg_proof_batch(self, commitments, zs, ys, proofs):
        """eth.VerifyKZGProof (eth/eth.go:114-135) over rows of bytes: (count, 48) commitments, (count, 32) little-endian z and y, (count, 48) proofs
        -> uint8 codes: 1 valid, 0 the pairing check failed, 2 z or y not below r, 3 commitment or proof not a valid G1 encoding"""
        c = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(-1, 48)
        pi = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 48)
        zs = np.ascontiguousarray(zs, dtype=np.uint8).reshape(-1, 32)
        ys = np.ascontiguousarray(ys, dtype=np.uint8).reshape(-1, 32)
        n = c.shape[0]
        if not (pi.shape[0] == zs.shape[0] == ys.shape[0] == n):
            raise KzgError(ERR_LEN_MISMATCH, "one commitment, z, y and proof per check")
        out = np.zeros(n, dtype=np.uint8)
        _chk(lib().kzg_hip_eth_verify_kzg_proof_batch(self.h, _p(c), _p(zs), _p(ys), _p(pi), n, _p(out)))
        return out

    def verify_kzg_proof_batch_combined(self, commitments, zs, ys, proofs, seed=None):
        """the same codes with one pairing check per group of rows (kzg_hip_eth_verify_kzg_proof_batch_combined): rows with code 2 or 3 drop out of
        their group's combination, the rows of a failing group are re-checked one by one.  seed as KZGSettings.check_proof_single_batch_combined"""
        c = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(-1, 48)
        pi = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 48)
        zs = np.ascontiguousarray(zs, dtype=np.uint8).reshape(-1, 32)
        ys = np.ascontiguousarray(ys, dtype=np.uint8).reshape(-1, 32)
        n = c.shape[0]
        if not (pi.shape[0] == zs.shape[0] == ys.shape[0] == n):
            raise KzgError(ERR_LEN_MISMATCH, "one commitment, z, y and proof per check")
        out = np.zeros(n, dtype=np.uint8)
        _chk(lib().kzg_hip_eth_verify_kzg_proof_batch_combined(self.h, _p(c), _p(zs), _p(ys), _p(pi), n, _seed32(seed), _p(out)))
        return out

    def kzg_to_versioned_hash_batch(self, commitments):
        """eth.KZGToVersionedHash (eth/eth.go:137-141) over (count, 48) uint8 commitments (any bytes: nothing is decoded) -> (count, 32) uint8"""
        c = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(-1, 48)
        out = np.zeros((c.shape[0], 32), dtype=np.uint8)
        _chk(lib().kzg_hip_eth_kzg_to_versioned_hash_batch(self.h, _p(c), c.shape[0], _p(out)))
        return out

    def kzg_to_versioned_hash_batch_dev(self, d_commitments, count, d_out):
        """the same on DEVICE pointers (integers; d_out 4-byte aligned), enqueued on the handle's stream without a host synchronisation"""
        _chk(lib().kzg_hip_eth_kzg_to_versioned_hash_batch_dev(self.h, d_commitments, count, d_out))

    PRECOMPILE_INPUT_LENGTH = 192
    CODE_INVALID_INPUT_LENGTH = 9   # of this binding only: the C ABI takes rows of 192 bytes and has no such code

    def point_evaluation_precompile_batch(self, inputs):
        """eth.PointEvaluationPrecompile (eth/eth.go:76-110) over a (count, 192) uint8 array or a list of byte strings (versioned hash 32 | z 32 LE |
        y 32 LE | commitment 48 | proof 48) -> uint8 codes: 1 valid (the reference returns precompile_return_value()), 0 "invalid kzg proof",
        4 "mismatched versioned hash", 2 z or y not below r, 3 commitment or proof not a valid G1 encoding, in the reference's order of checks
        (4, then 2, then 3).  A byte string of another length gets CODE_INVALID_INPUT_LENGTH = 9 ("invalid input length") here in the binding,
        without going to the device; the C ABI has no such code."""
        if isinstance(inputs, np.ndarray):
            rows = np.ascontiguousarray(inputs, dtype=np.uint8).reshape(-1, 192)
            out = np.zeros(rows.shape[0], dtype=np.uint8)
            _chk(lib().kzg_hip_eth_point_evaluation_precompile_batch(self.h, _p(rows), rows.shape[0], _p(out)))
            return out
        inputs = [bytes(b) for b in inputs]
        out = np.full(len(inputs), self.CODE_INVALID_INPUT_LENGTH, dtype=np.uint8)
        good = [i for i, b in enumerate(inputs) if len(b) == 192]
        if good:
            out[good] = self.point_evaluation_precompile_batch(np.frombuffer(b"".join(inputs[i] for i in good), dtype=np.uint8))
        elif not inputs:
            self.point_evaluation_precompile_batch(np.zeros((0, 192), dtype=np.uint8))   # (the empty call still needs the G2 setup)
        return out

    def point_evaluation_precompile_batch_dev(self, d_inputs, count, d_result):
        """the same on DEVICE pointers (integers), enqueued on the handle's stream without a host synchronisation"""
        _chk(lib().kzg_hip_eth_point_evaluation_precompile_batch_dev(self.h, d_inputs, count, d_result))

    def precompile_return_value(self):
        """precompileReturnValue (eth/globals.go:70-71): n and r as 32 big-endian bytes each"""
        out = C.create_string_buffer(64)
        _chk(lib().kzg_hip_eth_precompile_return_value(self.h, out))
        return out.raw

    def verify_kzg_commitments_against_transactions_batch(self, blocks, commitments):
        """eth.VerifyKZGCommitmentsAgainstTransactions (eth/eth.go:261-282) over many blocks: blocks[j] is the list of block j's serialized
        transactions (byte strings), commitments[j] its (k, 48) uint8 commitments (or a list of 48-byte strings) -> uint8 codes: 1 valid, 6 / 7 / 8
        the block's first malformed blob transaction (too short, also an empty transaction; offset out of bounds; trailing data no multiple of 32),
        5 the number of versioned hashes differs from the number of commitments, 4 a versioned hash does not match its commitment"""
        if len(blocks) != len(commitments):
            raise KzgError(ERR_LEN_MISMATCH, "one list of commitments per block")
        txs = [bytes(t) for b in blocks for t in b]
        offsets = np.zeros(len(txs) + 1, dtype=np.uint64)
        if txs:
            offsets[1:] = np.cumsum([len(t) for t in txs], dtype=np.uint64)
        data = np.frombuffer(b"".join(txs) or bytes(1), dtype=np.uint8)
        tx_counts = np.array([len(b) for b in blocks], dtype=np.uint64)
        comm = [np.frombuffer(b"".join(bytes(x) for x in c), dtype=np.uint8) if isinstance(c, (list, tuple)) else np.ascontiguousarray(c, dtype=np.uint8).reshape(-1)
                for c in commitments]
        if any(c.shape[0] % 48 for c in comm):
            raise KzgError(ERR_LEN_MISMATCH, "commitments of 48 bytes")
        comm_counts = np.array([c.shape[0] // 48 for c in comm], dtype=np.uint64)
        flat = np.ascontiguousarray(np.concatenate(comm + [np.zeros(48, dtype=np.uint8)]))
        out = np.zeros(len(blocks), dtype=np.uint8)
        _chk(lib().kzg_hip_eth_verify_kzg_commitments_against_transactions_batch(self.h, _p(data), _p(offsets), _p(tx_counts), _p(flat), _p(comm_counts), len(blocks),
                                                                                 _p(out)))
        return out

    def verify_aggregate_kzg_proof_batch(self, blobs, counts, commitments, proofs, intermediates=False):
        """eth.VerifyAggregateKZGProof (eth/eth.go:155-172) over many sidecars: `counts[j]` blobs (0 is valid) of the (sum(counts), n, 32) uint8 blobs and of
        the (sum(counts), 48) expected commitments belong to sidecar j, proofs is (sidecars, 48) -> uint8 codes: 1 valid, 0 the pairing check failed, 2 a
        field element of the block not below r, 3 a commitment or the proof not a valid G1 encoding.  intermediates=True: also the aggregated
        commitments (sidecars, 48), z and y (sidecars, 4) of every sidecar (unspecified where the code is 2 or 3)"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        s, total = counts.shape[0], int(counts.sum(dtype=object)) if counts.shape[0] else 0
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.n, 32)
        comm = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(-1, 48)
        pi = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 48)
        if blobs.shape[0] != total or comm.shape[0] != total or pi.shape[0] != s:
            raise KzgError(ERR_LEN_MISMATCH, "sum(counts) blobs and commitments, one proof per sidecar")
        out = np.zeros(s, dtype=np.uint8)
        c48, zs, ys = (np.zeros((s, 48), dtype=np.uint8), fr_empty(s), fr_empty(s)) if intermediates else (None, None, None)
        _chk(lib().kzg_hip_eth_verify_aggregate_kzg_proof_batch(self.h, _p(blobs), _p(counts), _p(comm), _p(pi), s, _p(out),
                                                                _p(c48) if intermediates else None, _p(zs) if intermediates else None,
                                                                _p(ys) if intermediates else None))
        return (out, c48, zs, ys) if intermediates else out

    def compute_aggregate_kzg_proof_batch(self, blobs, counts):
        """eth.ComputeAggregateKZGProof (eth/eth.go:175-182) over many sidecars in one call: `counts[j]` blobs (0 is valid) of the (sum(counts), n, 32)
        uint8 blobs belong to sidecar j -> ((sidecars, 48) proofs, (sum(counts), 48) commitments, (sidecars,) uint8 status).  status[j] is 0 where the
        row's outputs are those of compute_aggregate_kzg_proof on that sidecar alone, byte for byte; else ERR_BAD_BLOB / ERR_BAD_ARG (the status of
        the lone call), and the row's proof and commitments are zero bytes"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        s, total = counts.shape[0], int(counts.sum(dtype=object)) if counts.shape[0] else 0
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.n, 32)
        if blobs.shape[0] != total:
            raise KzgError(ERR_LEN_MISMATCH, "sum(counts) blobs")
        proofs, comm, status = np.zeros((s, 48), dtype=np.uint8), np.zeros((total, 48), dtype=np.uint8), np.zeros(s, dtype=np.uint8)
        _chk(lib().kzg_hip_eth_compute_aggregate_kzg_proof_batch(self.h, _p(blobs), _p(counts), s, _p(proofs), _p(comm), _p(status)))
        return proofs, comm, status

    def compute_aggregate_kzg_proof_batch_dev(self, d_blobs, counts, d_proofs, d_commitments, d_status):
        """the same on DEVICE pointers (integers; blobs 4-byte aligned, d_commitments may be None), enqueued on the handle's stream without a
        host synchronisation: the caller orders its own streams around the call; `counts` is a host array"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        _chk(lib().kzg_hip_eth_compute_aggregate_kzg_proof_batch_dev(self.h, d_blobs, _p(counts), counts.shape[0], d_proofs, d_commitments, d_status))

    def evaluate_polynomial_in_evaluation_form(self, polynomial, x):
        """eth.EvaluatePolynomialInEvaluationForm (eth/helpers.go:207-211)"""
        poly, x, y = _fr(polynomial), _fr(x), fr_empty(1)
        _chk(lib().kzg_hip_eth_evaluate_polynomial_in_evaluation_form(self.h, _p(poly), poly.shape[0], _p(x), _p(y)))
        return y[0]

    def compute_aggregate_kzg_proof(self, blobs):
        """eth.ComputeAggregateKZGProof (eth/eth.go:175-182) on (batch, n, 32) uint8 blobs (batch may be 0): (proof48, (batch, 48) commitments);
        KzgError "could not convert blobs to polynomials" / "invalid z challenge" like the reference"""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.n, 32)
        b = blobs.shape[0]
        proof, comm = np.zeros(48, dtype=np.uint8), np.zeros((b, 48), dtype=np.uint8)
        st = lib().kzg_hip_eth_compute_aggregate_kzg_proof(self.h, _p(blobs), b, _p(proof), _p(comm))
        if st == ERR_BAD_BLOB:
            raise KzgError(st, "could not convert blobs to polynomials")
        if st == ERR_BAD_ARG:
            raise KzgError(st, "invalid z challenge")
        _chk(st)
        return proof, comm

    def compute_aggregated_poly_and_commitment(self, blobs, commitments):
        """The prover-side pieces of eth.VerifyAggregateKZGProof (eth/eth.go:155-172): (aggregated polynomial (n, 4), aggregated commitment
        G1 image (18,), z (4,), y (4,)); the pairing of VerifyKZGProofFromPoints stays with the caller"""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.n, 32)
        comm = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(-1, 48)
        b = blobs.shape[0]
        if comm.shape[0] != b:
            raise KzgError(ERR_LEN_MISMATCH, "one commitment per blob")
        poly, c, z, y = fr_empty(self.n), g1_empty(1), fr_empty(1), fr_empty(1)
        st = lib().kzg_hip_eth_compute_aggregated_poly_and_commitment(self.h, _p(blobs), _p(comm), b, _p(poly), _p(c), _p(z), _p(y))
        if st == ERR_BAD_BLOB:
            raise KzgError(st, "could not convert blobs to polynomials")
        if st == ERR_BAD_POINT:
            raise KzgError(st, "invalid commitment")
        _chk(st)
        return poly, c[0], z[0], y[0]

    def bench_drop_in_proof(self, polys, threads, calls):
        """`threads` native host threads x `calls` blocking eth.ComputeKZGProof calls: (calls per second, each thread's last proof)"""
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        out, secs = np.zeros((threads, 48), dtype=np.uint8), C.c_double(0)
        _chk(lib().kzg_hip_bench_drop_in_eth_proof(self.h, _p(polys), polys.shape[1], polys.shape[0], threads, calls, _p(out), C.byref(secs)))
        return threads * calls / secs.value, out
