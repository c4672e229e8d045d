"""Memory images for the verification tests: the scalars of tests/verify_cases.py as the C ABI's Kilic images (points from the C oracle, which
shares no code with the kernels), G2 points with a chosen Jacobian Z, and eth.VerifyKZGProof's byte rows.  A plain helper module, imported by
name from tests/test_pairing_host.py (host emulation) and tests/test_gpu_verify.py (device)."""
import numpy as np

import pairing_ref as pr
import verify_cases as vc
from oracle import koracle as ko

P, R = pr.P, vc.R
R384 = pow(2, 384, P)


def u64s(v):
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]


def from_u64s(row):
    return sum(int(row[i]) << (64 * i) for i in range(6))


def rand_fp2(rng):
    return (rng.randrange(1, P), rng.randrange(1, P))


def g2_kilic(Q, z=(1, 0)):
    """affine reference point -> Kilic G2 image (3, 2, 6) of the Jacobian point (x z^2, y z^3, z); None or z == 0 -> Kilic's Zero() (0, 1, 0)"""
    if Q is None or z == (0, 0):
        return np.array([[u64s(0), u64s(0)], [u64s(R384), u64s(0)], [u64s(0), u64s(0)]], dtype=np.uint64)
    z2 = pr.f2sqr(z)
    coords = (pr.f2mul(Q[0], z2), pr.f2mul(Q[1], pr.f2mul(z2, z)), z)
    return np.array([[u64s(c * R384 % P) for c in coord] for coord in coords], dtype=np.uint64)


def g1_rescale(img, z):
    """the Kilic G1 image of the same point with Jacobian Z multiplied by z (an integer in [1, p))"""
    X, Y, Z = (from_u64s(row) for row in np.asarray(img).reshape(3, 6))
    return np.array([u64s(X * z * z % P), u64s(Y * z * z * z % P), u64s(Z * z % P)], dtype=np.uint64)


def g1_scalar(k, z=None):
    """[k] G1 from the oracle as a normalised image (Z = 1), or with Jacobian Z = z; infinity for k == 0 (mod r)"""
    if k % R == 0:
        return ko.g1_zero(1)[0]
    img = ko.g1_affine(ko.g1_mul(ko.g1_generator(), ko.fr_from_ints([k % R])[0]))[0]
    return img if z is None else g1_rescale(img, z)


def g1_affine_image(x, y):
    """the Kilic image of the affine point (x, y), on the curve or not: nothing is checked"""
    return np.array([u64s(x * R384 % P), u64s(y * R384 % P), u64s(R384)], dtype=np.uint64)


ORDER3 = (0, 2)      # on y^2 = x^3 + 4, of order 3: outside G1


def single_images(rows, rng):
    """rows of verify_cases.single_rows -> (commitments, proofs, xs, ys) images; C and pi alternate between Z = 1 and a random Jacobian Z"""
    cs = np.stack([g1_scalar(r[1], rng.randrange(2, P) if i % 2 else None) for i, r in enumerate(rows)])
    pis = np.stack([g1_scalar(r[2], rng.randrange(2, P) if i % 4 < 2 else None) for i, r in enumerate(rows)])
    return cs, pis, ko.fr_from_ints([r[3] for r in rows]), ko.fr_from_ints([r[4] for r in rows])


def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def compress_scalar(k):
    return ko.g1_compress(g1_scalar(k)[None])[0]


def curve_point_outside_g1():
    """a point of y^2 = x^3 + 4 over F_p whose order does not divide r (most points: the cofactor is 0x396c8c005555e1568c00aaab0000aaab)"""
    for x in range(1, 100):
        rhs = (x * x * x + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs and pr.g1_mul((x, y), R) is not None:
            return (x, y)
    raise AssertionError("no such point below x = 100")


def compress_affine(pt):   # ZCash form of an affine point, whatever its order
    b = bytearray(pt[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if pt[1] > (P - 1) // 2 else 0)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def eth_rows(s, rng):
    """[(name, commitment48, z32, y32, proof48, code)]: every single row of verify_cases compressed by the oracle (code 1 / 0 from its truth
    value), and byte-level rows with the code the reference's order of checks gives (eth/eth.go:114-133: z, then y, then commitment, then proof)"""
    rows = [(name, compress_scalar(c), le32(x), le32(y), compress_scalar(t), 1 if want else 0)
            for name, c, t, x, y, want in vc.single_rows(s, rng)]
    inf = np.frombuffer(bytes([0xc0]) + bytes(47), dtype=np.uint8)
    z = vc.rand_fr(rng)
    rows.append(("bytes/zero_blob", inf, le32(z), le32(0), inf, 1))
    rows.append(("bytes/zero_blob_y=1", inf, le32(z), le32(1), inf, 0))
    t = vc.rand_fr(rng)
    c = (R - 1 + (s - (R - 1)) * t) % R
    rows.append(("bytes/z=y=r-1", compress_scalar(c), le32(R - 1), le32(R - 1), compress_scalar(t), 1))
    rows.append(("bytes/z=y=r-1_c+1", compress_scalar(c + 1), le32(R - 1), le32(R - 1), compress_scalar(t), 0))
    # a valid row to spoil
    t, x, y = vc.rand_fr(rng), vc.rand_fr(rng), vc.rand_fr(rng)
    good_c, good_pi = compress_scalar(y + (s - x) * t), compress_scalar(t)
    rows.append(("bytes/valid", good_c, le32(x), le32(y), good_pi, 1))
    undecodable = np.frombuffer(bytes([0x80]) + bytes(47), dtype=np.uint8)          # x = 0: (0, 2), on the curve, of order 3
    rows.append(("bytes/z=r_and_bad_commitment", undecodable, le32(R), le32(y), good_pi, 2))
    rows.append(("bytes/y=r_and_bad_proof", good_c, le32(x), le32(R), undecodable, 2))
    rows.append(("bytes/z=2^256-1", good_c, le32(2 ** 256 - 1), le32(y), good_pi, 2))
    rows.append(("bytes/y=r", good_c, le32(x), le32(R), good_pi, 2))
    rows.append(("bytes/proof_outside_g1", good_c, le32(x), le32(y), compress_affine(curve_point_outside_g1()), 3))
    rows.append(("bytes/proof_order_3", good_c, le32(x), le32(y), undecodable, 3))
    xp = bytearray(P.to_bytes(48, "big")); xp[0] |= 0x80
    rows.append(("bytes/proof_x=p", good_c, le32(x), le32(y), np.frombuffer(bytes(xp), dtype=np.uint8), 3))
    rows.append(("bytes/proof_0x40", good_c, le32(x), le32(y), np.frombuffer(bytes([0x40]) + bytes(47), dtype=np.uint8), 3))
    rows.append(("bytes/proof_0xe0", good_c, le32(x), le32(y), np.frombuffer(bytes([0xe0]) + bytes(47), dtype=np.uint8), 3))
    rows.append(("bytes/commitment_outside_g1", compress_affine(curve_point_outside_g1()), le32(x), le32(y), good_pi, 3))
    rows.append(("bytes/commitment_uncompressed_flag", np.frombuffer(bytes([good_c[0] & 0x7f]) + bytes(good_c[1:]), dtype=np.uint8), le32(x), le32(y), good_pi, 3))
    return rows


def eth_arrays(rows):
    return tuple(np.ascontiguousarray(np.stack([r[k] for r in rows])) for k in (1, 2, 3, 4))
