"""Rows, masks and erasure lists shared by tests/test_recovery_batch_host.py and tests/test_gpu_recovery_batch.py (built from the oracle only)."""
import numpy as np

from oracle import koracle as ko

OK, ERR_BAD_ARG, ERR_RECOVERY = 0, 5, 10


def data_rows(ofs, n, rows, seed, full_degree=()):
    """evaluations of `rows` polynomials whose upper half of coefficients is zero (recover_from_samples_test.go:62-137); rows listed in full_degree keep all n"""
    out = np.zeros((rows, n, 4), dtype=np.uint64)
    for r in range(rows):
        poly = ko.synthetic_blob(seed + r, n)
        if r not in full_degree:
            poly[n // 2:] = 0
        out[r] = ofs.fft(poly) if n > 1 else poly
    return out


def mask(n, missing, rng):
    """n bytes with `missing` zeros at random places"""
    m = np.ones(n, dtype=np.uint8)
    m[rng.permutation(n)[:missing]] = 0
    return m


def ragged_counts(n):
    """missing counts of one call: nothing, one, around half, all but one -- and a row with nothing present in the middle"""
    return [0, 1, n // 2 - 1, n, n // 2, n // 2 + 1, n - 1]


def ragged_masks(n, rows, rng):
    counts = ragged_counts(n)
    return np.stack([mask(n, counts[r % len(counts)], rng) for r in range(rows)])


def blanked(samples, present):
    """the samples as a caller holds them: zeros where nothing is present"""
    s = samples.copy()
    s[np.broadcast_to(present, s.shape[:2]) == 0] = 0
    return s


def oracle_row(ofs, samples, present):
    """(status, row) the oracle gives for one row, None where it refuses the row"""
    try:
        return OK, ofs.recover_poly_from_samples(samples, present)
    except ko.OracleError:
        return None, None
