"""Rows of (polynomial, z) for eth.ComputeKZGProof (eth/helpers.go:179-203) and what the reference returns for them, in Python integers.

A row is a polynomial p in EVALUATION form on the bit-reversed domain of size n (DomainFr, eth/globals.go:61-66) and a challenge z.  The secret
s of the setup is known to the tests (1337 for the committed 4096-point Lagrange setup, S_TEST for the generated ones), so the proof is a known
multiple of the generator and no quotient has to be formed:

    coeffs = inverse transform of bitrev(p)            y = p(z)            proof = [d] G1,  d = (p(s) - y) / (s - z)  (mod r)

and a row whose z lies in the domain is refused ("invalid z challenge", :190-192): ok = False, proof and y all zero.  Nothing here inverts in
batches, and nothing of the product is imported: the transform and Horner's rule are oracle/pyref.py's, the one scalar multiplication and the
compression oracle/koracle.py's.  Every row keeps z != s (the identity divides by s - z).

literal_proof() is eth/helpers.go:179-203 as written (quotient q_i = (p_i - y) / (w_i - z), then bls.LinCombG1 over the bit-reversed Lagrange
points): tests/test_eth_rows.py shows that the two agree.  lagrange_setup() builds the Lagrange setup of any size from the secret, and
split_form() restates the dispatch rule of launch_eth_quotient (csrc/k_fr.hip) so that a test can say which kernels a shape runs.
"""
import functools
import json
import os

import numpy as np

from oracle import koracle as ko
from oracle import pyref

R = pyref.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S_TEST = int(json.load(open(os.path.join(GOLDEN, "reference_kats.json")))["test_secret"]["value"]) % R
S_GOLDEN = 1337                                   # secret of tests/golden/trusted_setup_g1_lagrange.bin
ZERO_PROOF = bytes([0xC0]) + bytes(47)            # the compressed point at infinity

# eth_quotient_scratch_elems (csrc/k_fr.hip), the condition under which NO row-split scratch is asked for, as it stands in the source
SPLIT_RULE_SOURCE = "if (one_wg || n < 2048 || (n & (n - 1)) != 0 || S > 64 || batch * S > 256) return 0;"


def split_form(n, batch):
    """True: k_eth_quotient_parts + k_eth_quotient_finish (a row over S = n / 1024 workgroups); False: k_eth_quotient (one workgroup per row)"""
    S = n // 1024
    return n >= 2048 and n & (n - 1) == 0 and S <= 64 and batch * S <= 256


def ilog2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def root_of_unity(n):
    return pow(7, (R - 1) // n, R)                # bls/globals.go:24-60


@functools.lru_cache(maxsize=None)
def domain(n):
    """DomainFr: the n-th roots of unity in bit-reversed order"""
    w, bits = root_of_unity(n), ilog2(n)
    return [pow(w, pyref.rev_bits(i, bits), R) for i in range(n)]


@functools.lru_cache(maxsize=None)
def _pfs(scale):
    return pyref.FFTSettings(scale)


def coefficients(n, poly):
    return _pfs(ilog2(n)).fft(pyref.bitrev(list(poly)), inv=True)


class Reference:
    """expected(poly, z) for one size and secret; a polynomial's coefficients and p(s) are kept, so rows that share a polynomial pay one transform"""

    def __init__(self, n, s):
        self.n, self.s, self.dom = n, s % R, domain(n)
        self.in_domain = set(self.dom)
        self._polys = {}

    def poly_facts(self, poly):
        key = tuple(poly)
        if key not in self._polys:
            c = coefficients(self.n, key)
            self._polys[key] = (c, pyref.eval_poly(c, self.s))
        return self._polys[key]

    def y(self, poly, z):
        return pyref.eval_poly(self.poly_facts(poly)[0], z % R)

    def dlog(self, poly, z):
        z %= R
        assert z != self.s
        _, at_s = self.poly_facts(poly)
        return (at_s - self.y(poly, z)) * pow(self.s - z, -1, R) % R

    def expected(self, poly, z):
        """(ok, y, 48 proof bytes)"""
        if z % R in self.in_domain:
            return False, 0, bytes(48)
        d = self.dlog(poly, z)
        return True, self.y(poly, z), ko.g1_compress(ko.g1_mul(ko.g1_generator(), ko.fr_from_ints([d])[0]))[0].tobytes()


def lagrange_dlogs(n, s):
    """L_i(s) = w_i (s^n - 1) / (n (s - w_i)), i in natural order of the domain"""
    w = root_of_unity(n)
    num = (pow(s, n, R) - 1) % R
    out = []
    for i in range(n):
        wi = pow(w, i, R)
        assert wi != s % R
        out.append(wi * num % R * pow(n * (s - wi) % R, -1, R) % R)
    return out


@functools.lru_cache(maxsize=None)
def lagrange_setup(n, s=S_TEST):
    """[L_i(s)] G1 in NATURAL order, as kzg_hip_eth_settings_new takes it (it applies the bit reversal of eth/globals.go:48 itself): (n, 3, 6) images"""
    g = ko.g1_generator()
    ks = ko.fr_from_ints(lagrange_dlogs(n, s))
    return np.stack([ko.g1_mul(g, ks[i]) for i in range(n)])


def golden_lagrange_setup():
    return ko.g1_decompress(np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))


def literal_proof(n, poly, z, lagrange_natural):
    """eth/helpers.go:179-203 as written: (ok, y, 48 proof bytes) with y from the barycentric formula and the proof from the quotient's commitment"""
    dom, z = domain(n), z % R
    if z in dom:
        return False, 0, bytes(48)
    y = pyref.eval_in_evaluation_form(list(poly), z, dom)
    q = [(p - y) * pow(w - z, -1, R) % R for p, w in zip(poly, dom)]
    lag_br = ko.reverse_bit_order(lagrange_natural) if n > 1 else lagrange_natural
    return True, y, ko.g1_compress(ko.lincomb_g1(lag_br, ko.fr_from_ints(q)))[0].tobytes()


def rand_fr(rng):
    return rng.randrange(R)


def rand_poly(rng, n):
    return tuple(rng.randrange(R) for _ in range(n))


# lanes of the one-workgroup kernel whose four slots i = tid + 1024 k get a domain element as z
SLOT_LANES = (0, 63, 64, 1023)


def named_rows(n, s, rng, pool=None):
    """[(name, poly, z)]: the crafted rows that exist at this size.  `pool`: random polynomials to draw from (their transforms are shared between
    rows and batches); rows that need a polynomial of their own build one."""
    dom = domain(n)
    pool = pool or [rand_poly(rng, n) for _ in range(4)]
    pick = lambda: pool[rng.randrange(len(pool))]
    rows = []

    def put(name, poly, z):
        z %= R
        assert z != s % R and len(poly) == n
        rows.append((name, tuple(poly), z))

    def outside():                                  # a full-width z outside the domain
        while True:
            z = rng.randrange(R)
            if pow(z, n, R) != 1 and z != s % R:
                return z
    put("random_z", pick(), outside())
    put("z=0", pick(), 0)
    put("z=1_in_domain", pick(), 1)
    put("z=r-1" + ("_in_domain" if n >= 2 else ""), pick(), R - 1)
    for tid in SLOT_LANES:
        for k in range(4):
            i = tid + 1024 * k
            if i < n:
                put("domain_slot%d_lane%d" % (k, tid), pick(), dom[i])
    if n > 4096:                                    # the last block of 4096 of a longer row: its first, an inner and its last element
        for i in (n - 4096, n - 4096 + 1024 + 63, n - 1):
            put("domain_last_block_%d" % i, pick(), dom[i])
    elif n > 1:
        put("domain_last_element", pick(), dom[n - 1])
    put("z^n=-1", pick(), root_of_unity(2 * n) if n > 1 else R - 1)            # a primitive 2n-th root of unity: outside the domain
    put("z^n=-1_odd_power", pick(), pow(root_of_unity(2 * n), 2 * rng.randrange(n) + 1, R))
    put("zero_polynomial", (0,) * n, outside())
    put("zero_polynomial_z=0", (0,) * n, 0)
    c = rng.randrange(1, R)
    put("constant_polynomial", (c,) * n, outside())
    put("constant_r-1", (R - 1,) * n, outside())
    # entries r - 1 among random ones, first and last positions included
    p = list(pick())
    for i in {0, n - 1, n // 2, min(n - 1, 1023), min(n - 1, 1024)}:
        p[i] = R - 1
    put("entries_r-1", p, outside())
    # p_j == y for one j: p' = p - (p_j - y) (x - z) / (w_j - z) keeps p'(z) = y and moves the value at w_j onto it
    if n >= 2:
        ref = Reference(n, s)
        base, z = pick(), outside()
        y = ref.y(base, z)
        for j in sorted({0, n - 1, n // 3}):
            f = (base[j] - y) * pow(dom[j] - z, -1, R) % R
            p = [(v - f * (w - z)) % R for v, w in zip(base, dom)]
            assert p[j] == y
            put("value_at_%d_equals_y" % j, p, z)
    put("invalid_with_zero_polynomial", (0,) * n, dom[n // 2])
    return rows


def _ordinary(n, s, rng, pool):
    while True:
        z = rng.randrange(R)
        if pow(z, n, R) != 1 and z != s % R:
            return ("ordinary", pool[rng.randrange(len(pool))] if pool else rand_poly(rng, n), z)


def batch_of(n, batch, s, rng, boundaries=(), pool=None):
    """`batch` rows [(name, poly, z)]: the named rows in rotation (fresh random ones each time round) with ordinary rows between them, an
    invalid row pinned on the first row, on the last row and on the row below each boundary, and a valid crafted one on the row above it"""
    rows = []
    while len(rows) < batch:
        named = named_rows(n, s, rng, pool)
        rot = rng.randrange(len(named))
        for row in named[rot:] + named[:rot]:       # an ordinary row after every crafted one
            rows += [row, _ordinary(n, s, rng, pool)]
    rows = rows[:batch]
    named = named_rows(n, s, rng, pool)
    invalid = [r_ for r_ in named if pow(r_[2], n, R) == 1]
    valid = [r_ for r_ in named if pow(r_[2], n, R) != 1]
    pins = {0: invalid[0], batch - 1: invalid[-1]}
    for b in boundaries:
        if 0 < b < batch:
            pins[b - 1] = invalid[(b + 1) % len(invalid)]
            pins[b] = valid[b % len(valid)]
    if batch == 1:
        pins = {}
    for at, row in pins.items():
        rows[at] = row
    return rows


@functools.lru_cache(maxsize=256)
def _poly_image(poly):
    return ko.fr_from_ints(poly)


def to_arrays(rows):
    """(batch, n, 4) polynomials and (batch, 4) challenges as Montgomery images"""
    polys = np.stack([_poly_image(p) for _, p, _ in rows])
    zs = ko.fr_from_ints([z for _, _, z in rows])
    return polys, zs
