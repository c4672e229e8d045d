"""Plain-Python reference of the BLS12-381 pairing, for the tests of tower.hpp / g2.hpp / pairing.hpp.

Deliberately built differently from the device code so that the two check each other:
  * F_p12 is F_p[w] / (w^12 - 2 w^6 + 2), a flat polynomial ring (u = w^6 - 1, v = w^2), not the tower;
  * the Miller loop runs on AFFINE twist points (one F_p2 inversion per step) and evaluates the untwisted lines
    l(P) = yP - lambda w^-1 xP + lambda w^-3 xT - yT w^-3 directly in F_p12;
  * the final exponentiation is a plain pow by (p^12 - 1) / r.
Integers only; imports nothing of the product.
"""
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
X_ABS = 0xd201000000010000          # BLS parameter x = -X_ABS
FINAL_EXP = (P ** 12 - 1) // R


# ---------------- F_p2 = F_p[u] / (u^2 + 1), elements (c0, c1) ----------------
def f2add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def f2sub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
def f2neg(a): return ((-a[0]) % P, (-a[1]) % P)
def f2mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
def f2sqr(a): return f2mul(a, a)
def f2inv(a):
    d = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * d % P, (-a[1]) * d % P)
def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1: r = f2mul(r, a)
        a = f2sqr(a); e >>= 1
    return r
def f2sqrt(a):
    """a square root of a in F_p2, or None: Tonelli-Shanks in F_p2^* (order p^2 - 1 = 2^s q)"""
    if a == (0, 0): return (0, 0)
    order = P * P - 1
    s, q = 0, order
    while q % 2 == 0: q //= 2; s += 1
    if f2pow(a, order // 2) != (1, 0): return None
    z = (1, 1)
    while f2pow(z, order // 2) == (1, 0): z = (z[0] + 1, 1)
    m, c, t, r = s, f2pow(z, q), f2pow(a, q), f2pow(a, (q + 1) // 2)
    while t != (1, 0):
        i, tt = 0, t
        while tt != (1, 0): tt = f2sqr(tt); i += 1
        b = c
        for _ in range(m - i - 1): b = f2sqr(b)
        m, c = i, f2sqr(b)
        t, r = f2mul(t, c), f2mul(r, b)
    return r


# ---------------- G2 on E': y^2 = x^3 + 4 (u + 1), affine, None = infinity ----------------
B2 = (4, 4)
G2_GEN = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
           0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
          (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
           0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))
G1_GEN = (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
          0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)


def g2_on_curve(Q):
    return Q is None or f2sqr(Q[1]) == f2add(f2mul(f2sqr(Q[0]), Q[0]), B2)
def g2_neg(Q): return None if Q is None else (Q[0], f2neg(Q[1]))
def g2_add(A, B):
    if A is None: return B
    if B is None: return A
    if A[0] == B[0]:
        if A[1] != B[1] or A[1] == (0, 0): return None
        lam = f2mul(f2mul((3, 0), f2sqr(A[0])), f2inv(f2add(A[1], A[1])))
    else:
        lam = f2mul(f2sub(B[1], A[1]), f2inv(f2sub(B[0], A[0])))
    x = f2sub(f2sub(f2sqr(lam), A[0]), B[0])
    return (x, f2sub(f2mul(lam, f2sub(A[0], x)), A[1]))
def g2_mul(Q, k):
    acc = None
    for bit in bin(k)[2:] if k > 0 else "":
        acc = g2_add(acc, acc)
        if bit == "1": acc = g2_add(acc, Q)
    return acc
def g1_add(A, B):
    if A is None: return B
    if B is None: return A
    if A[0] == B[0]:
        if A[1] != B[1] or A[1] == 0: return None
        lam = 3 * A[0] * A[0] * pow(2 * A[1], P - 2, P) % P
    else:
        lam = (B[1] - A[1]) * pow(B[0] - A[0], P - 2, P) % P
    x = (lam * lam - A[0] - B[0]) % P
    return (x, (lam * (A[0] - x) - A[1]) % P)
def g1_mul(Pt, k):
    acc = None
    for bit in bin(k)[2:] if k > 0 else "":
        acc = g1_add(acc, acc)
        if bit == "1": acc = g1_add(acc, Pt)
    return acc


def _larger(y):  # ZCash "lexicographically largest" for F_p2: c1 decides, c0 when c1 == 0
    return y[1] > (P - 1) // 2 if y[1] else y[0] > (P - 1) // 2
def g2_compress(Q):
    if Q is None: return bytes([0xc0]) + bytes(95)
    b = bytearray(Q[0][1].to_bytes(48, "big") + Q[0][0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if _larger(Q[1]) else 0)
    return bytes(b)
def g2_decompress(b):
    """the point, or raises ValueError (flags, x >= p, not on the curve, not in the subgroup)"""
    if len(b) != 96 or not b[0] & 0x80: raise ValueError("not compressed")
    if b[0] & 0x40:
        if b[0] & 0x3f or any(b[1:]): raise ValueError("bad infinity")
        return None
    x1 = int.from_bytes(bytes([b[0] & 0x1f]) + b[1:48], "big"); x0 = int.from_bytes(b[48:], "big")
    if x0 >= P or x1 >= P: raise ValueError("x >= p")
    x = (x0, x1)
    y = f2sqrt(f2add(f2mul(f2sqr(x), x), B2))
    if y is None: raise ValueError("not on the curve")
    if _larger(y) != bool(b[0] & 0x20): y = f2neg(y)
    if g2_mul((x, y), R) is not None: raise ValueError("not in the subgroup")
    return (x, y)


# ---------------- F_p12 = F_p[w] / (w^12 - 2 w^6 + 2), elements: tuples of 12 ints ----------------
ONE12 = (1,) + (0,) * 11
def f12mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b): t[i + j] += x * y
    for k in range(22, 11, -1):             # w^k = 2 w^(k-6) - 2 w^(k-12)
        c = t[k]
        if c: t[k - 6] += 2 * c; t[k - 12] -= 2 * c
    return tuple(v % P for v in t[:12])
def f12pow(a, e):
    r = ONE12
    for bit in bin(e)[2:]:
        r = f12mul(r, r)
        if bit == "1": r = f12mul(r, a)
    return r
def f12inv(a): return f12pow(a, P ** 12 - 2)
def f2_to_12(a):  # a0 + a1 u, u = w^6 - 1
    t = [0] * 12; t[0] = (a[0] - a[1]) % P; t[6] = a[1] % P
    return tuple(t)
def w_pow(k):
    t = [0] * 12
    if k >= 0:
        t[k % 12] = 1
        return f12pow(tuple(t), 1) if k < 12 else f12pow(tuple([0, 1] + [0] * 10), k)
    return f12inv(w_pow(-k))
def from_tower(c):
    """tower element as 6 F_p2 values (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) -> flat form (w^(i + 2j) for c_i.c_j)"""
    out = (0,) * 12
    for i in range(2):
        for j in range(3):
            term = f12mul(f2_to_12(c[3 * i + j]), w_pow(i + 2 * j))
            out = tuple((x + y) % P for x, y in zip(out, term))
    return out
def to_tower(a):
    """inverse of from_tower: solves the 12 x 12 linear system column by column (basis images precomputed)"""
    basis = []
    for k in range(12):
        c = [(0, 0)] * 6; c[k // 2] = (1, 0) if k % 2 == 0 else (0, 1)
        basis.append(from_tower(c))
    # Gaussian elimination over F_p: solve sum_k x_k basis[k] = a
    m = [[basis[k][row] for k in range(12)] + [a[row]] for row in range(12)]
    for col in range(12):
        piv = next(r for r in range(col, 12) if m[r][col])
        m[col], m[piv] = m[piv], m[col]
        iv = pow(m[col][col], P - 2, P)
        m[col] = [v * iv % P for v in m[col]]
        for r in range(12):
            if r != col and m[r][col]:
                f = m[r][col]; m[r] = [(x - f * y) % P for x, y in zip(m[r], m[col])]
    x = [m[k][12] for k in range(12)]
    return [(x[2 * k], x[2 * k + 1]) for k in range(6)]


_W_INV1, _W_INV3 = None, None
def _line(T, lam, Pt):
    """l(P) for the untwisted line of slope lam (twist coordinates) through T: yP - lam w^-1 xP + (lam xT - yT) w^-3"""
    global _W_INV1, _W_INV3
    if _W_INV1 is None: _W_INV1, _W_INV3 = w_pow(-1), w_pow(-3)
    l = [0] * 12; l[0] = Pt[1]
    l = tuple(l)
    a = f12mul(f12mul(f2_to_12(lam), _W_INV1), tuple([(-Pt[0]) % P] + [0] * 11))
    b = f12mul(f2_to_12(f2sub(f2mul(lam, T[0]), T[1])), _W_INV3)
    return tuple((x + y + z) % P for x, y, z in zip(l, a, b))
def miller_loop(Pt, Q):
    """f_{|x|, Q}(P), conjugated for the negative x (the inverse up to factors the final exponentiation removes)"""
    if Pt is None or Q is None: return ONE12
    f, T = ONE12, Q
    for bit in bin(X_ABS)[3:]:
        lam = f2mul(f2mul((3, 0), f2sqr(T[0])), f2inv(f2add(T[1], T[1])))
        f = f12mul(f12mul(f, f), _line(T, lam, Pt)); T = g2_add(T, T)
        if bit == "1":
            lam = f2mul(f2sub(Q[1], T[1]), f2inv(f2sub(Q[0], T[0])))
            f = f12mul(f, _line(T, lam, Pt)); T = g2_add(T, Q)
    return f12pow(f, P ** 6)   # conjugation = Frobenius p^6
def pairing(Pt, Q, exponent=FINAL_EXP):
    return f12pow(miller_loop(Pt, Q), exponent)
def multi_pairing(pairs, exponent=FINAL_EXP):
    f = ONE12
    for Pt, Q in pairs: f = f12mul(f, miller_loop(Pt, Q))
    return f12pow(f, exponent)
