"""Crafted rows for the proof checks (k_kzg_check_inputs / k_eth_check_inputs, capi_verify.hip), as SCALARS.

Every input of a check is written as a multiple of the generator: C = [c] G1, pi = [t] G1, and the secret s of the setup is known to the
tests.  Then the single check e(C - [y] G1, G2) == e(pi, [s - x] G2) holds iff  c - y + (x - s) t == 0 (mod r), and the multi check over
n values iff  c - I'(s) + (x^np - s^n) t == 0 (mod r), with np = next_pow2(n) and I' the reference's interpolation polynomial of the
zero-padded values (fft_fr.go:60-68, kzg_multi_proofs.go:55-72).  Truth is one line of modular arithmetic; nothing of the product is imported.

Row names are "<class>/<variant>"; SINGLE_CLASSES / MULTI_CLASSES list the classes and whether both truth values exist for them.
"""
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
LAMBDA = 0xac45a4010001a40200000000ffffffff      # phi(P) = [LAMBDA] P on G1
HL = LAMBDA // 2                                 # the split's |k1| <= HL (glv_split_signed, g1.hpp)
K2_MAX = ((R - 1) // 2 + HL) // LAMBDA           # ... and k2 <= K2_MAX

# class -> True when the class has a valid and an invalid variant
SINGLE_CLASSES = {"ordinary": True, "constant": True, "edge_x": True, "edge_y": True, "add_doubles": True, "add_cancels": False,
                  "sub_doubles": True, "sub_cancels": True, "generator": True}
MULTI_CLASSES = {"ordinary": True, "pi_inf": True, "c_is_interp": True, "add_doubles": True, "add_cancels": False, "sub_doubles": True,
                 "x_zero": True, "x_one": True}
MULTI_NS = (1, 2, 8, 32, 3, 5, 12)


def glv_split(k):
    """glv_split_signed on Python integers: (|k1|, k2, neg1, neg2) with k == +-|k1| +- k2 LAMBDA (mod r)"""
    sg = k > (R - 1) // 2
    a = R - k if sg else k
    q = (a + HL) // LAMBDA
    k1 = a - q * LAMBDA
    return abs(k1), q, sg ^ (k1 < 0), sg


def edge_scalars():
    """(name, k): the scalars of the issue's list, and those whose signed split has a zero or a maximal half"""
    q_hi = ((R - 1) // 2 - HL) // LAMBDA          # the largest q with q LAMBDA + HL <= (r - 1) / 2
    out = [("0", 0), ("1", 1), ("r-1", R - 1), ("lambda", LAMBDA), ("r-lambda", R - LAMBDA), ("lambda-1", LAMBDA - 1),
           ("k1_zero", LAMBDA * 0x1234567890abcdef0123456789abcdef % R),      # (0, m)
           ("k2_zero_k1_max", HL),                                              # (HL, 0): the largest scalar with no phi half
           ("k1_min", HL + 1),                                                  # (-HL, 1)
           ("k2_max", (R - 1) // 2), ("k2_max_neg", (R + 1) // 2),              # (., K2_MAX), both signs
           ("both_max", q_hi * LAMBDA + HL), ("both_max_neg", R - (q_hi * LAMBDA + HL)),
           ("k2_max_k1_-1", (R - 1) // 2 - 1)]                                   # (r - 1) / 2 == K2_MAX LAMBDA exactly: its split is (0, K2_MAX)
    return out


def rand_fr(rng):
    return rng.randrange(1, R)


def inv(a):       # bls.InvModFr: inv(0) = 0
    return pow(a, R - 2, R)


def single_want(s, c, t, x, y):
    return (c - y + (x - s) * t) % R == 0


def single_rows(s, rng):
    """[(name, c, t, x, y, want)]; scalars that a class does not fix are full-width random"""
    s %= R
    rows = []

    def put(name, c, t, x, y):
        c, t, x, y = c % R, t % R, x % R, y % R
        rows.append((name, c, t, x, y, single_want(s, c, t, x, y)))

    def valid_c(t, x, y):
        return y + (s - x) * t

    # ordinary: full-width x, y, t
    for k in range(3):
        t, x, y = rand_fr(rng), rand_fr(rng), rand_fr(rng)
        c = valid_c(t, x, y)
        put("ordinary/valid%d" % k, c, t, x, y)
        put("ordinary/y+1_%d" % k, c, t, x, y + 1)
        put("ordinary/x+1_%d" % k, c, t, x + 1, y)
        put("ordinary/t+1_%d" % k, c, t + 1, x, y)
    # constant polynomial: pi = inf
    x, y = rand_fr(rng), rand_fr(rng)
    put("constant/valid", y, 0, x, y)
    put("constant/c=y+1", y + 1, 0, x, y)
    put("constant/all_zero", 0, 0, x, 0)
    put("constant/all_zero_x_zero", 0, 0, 0, 0)
    # edge scalars as x and as y
    for name, e in edge_scalars():
        t, x, y = rand_fr(rng), rand_fr(rng), rand_fr(rng)
        put("edge_x/%s_valid" % name, valid_c(t, e, y), t, e, y)
        put("edge_x/%s_c+1" % name, valid_c(t, e, y) + 1, t, e, y)
        put("edge_y/%s_valid" % name, valid_c(t, x, e), t, x, e)
        put("edge_y/%s_t+1" % name, valid_c(t, x, e), t + 1, x, e)
    for nx, ex in edge_scalars()[:6]:               # both at once
        for ny, ey in edge_scalars()[:3]:
            t = rand_fr(rng)
            put("edge_x/%s_with_y_%s_valid" % (nx, ny), valid_c(t, ex, ey), t, ex, ey)
    # the final addition doubles: C - E == [x] pi
    t, y = rand_fr(rng), rand_fr(rng)
    x = s * inv(2) % R
    put("add_doubles/x=s/2", y + x * t, t, x, y)
    x = rand_fr(rng)
    put("add_doubles/other_x", y + x * t, t, x, y)
    put("add_doubles/y_zero", x * t, t, x, 0)
    # the final addition cancels: C - E == -[x] pi (never valid: the sum is inf, -pi is not)
    for k in range(2):
        t, x, y = rand_fr(rng), rand_fr(rng), rand_fr(rng)
        put("add_cancels/%d" % k, y - x * t, t, x, y)
    # the subtraction doubles: C == -E
    x, y = rand_fr(rng), rand_fr(rng)
    c = -y % R
    t = 2 * c * inv((s - x) % R) % R
    put("sub_doubles/valid", c, t, x, y)
    put("sub_doubles/t+1", c, t + 1, x, y)
    # the subtraction cancels: C == E.  At x = s any proof is valid (the reference's [s - x] G2 is infinity)
    t, y = rand_fr(rng), rand_fr(rng)
    put("sub_cancels/x=s", y, t, s, y)
    put("sub_cancels/other_x", y, t, rand_fr(rng), y)
    put("sub_cancels/x_zero", y, t, 0, y)
    # everything is the generator, and neighbours
    put("generator/x=s", 1, 1, s, 1)
    put("generator/x=1", 1, 1, 1, 1)
    put("generator/x_random", 1, 1, rand_fr(rng), 1)
    put("generator/c=2", 2, 1, s - 1, 1)
    put("generator/y=2", 1, 1, s + 1, 2)
    put("generator/pi=-G", 1, R - 1, s, 1)
    put("generator/pi=-G_x=1", 1, R - 1, 1, 1)
    return rows


def next_pow2(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def root_of_unity(n):   # the reference's root of the n-point domain, n a power of two (bls/globals.go:24-60)
    assert n & (n - 1) == 0
    return pow(7, (R - 1) // n, R)


def interp_at(ys, x, at):
    """I'(at): the naive inverse DFT of ys zero-padded to np values, coefficient i times x^-i (0^-1 = 0), evaluated at `at`"""
    npad = next_pow2(len(ys))
    vals = [v % R for v in ys] + [0] * (npad - len(ys))
    w_inv = inv(root_of_unity(npad))
    n_inv = inv(npad)
    xi = inv(x % R)
    acc = 0
    for i in range(npad):
        coef = sum(v * pow(w_inv, i * j, R) for j, v in enumerate(vals)) * n_inv % R
        acc += coef * pow(xi, i, R) * pow(at, i, R)      # pow(., 0) == 1 also for 0
    return acc % R


def multi_want(s, c, t, x, ys):
    n = len(ys)
    return (c - interp_at(ys, x, s) + (pow(x, next_pow2(n), R) - pow(s, n, R)) * t) % R == 0


def multi_rows(s, rng):
    """[(name, c, t, x, ys, n, want)], every n of MULTI_NS in the ordinary class; ys full-width random"""
    s %= R
    rows = []

    def put(name, c, t, x, ys):
        c, t, x, ys = c % R, t % R, x % R, [v % R for v in ys]
        rows.append((name, c, t, x, ys, len(ys), multi_want(s, c, t, x, ys)))

    def valid_c(t, x, ys):
        n = len(ys)
        return interp_at(ys, x, s) - (pow(x, next_pow2(n), R) - pow(s, n, R)) * t

    def rand_ys(n):
        return [rand_fr(rng) for _ in range(n)]

    for n in MULTI_NS:
        t, x, ys = rand_fr(rng), rand_fr(rng), rand_ys(n)
        c = valid_c(t, x, ys)
        put("ordinary/n%d_valid" % n, c, t, x, ys)
        put("ordinary/n%d_c+1" % n, c + 1, t, x, ys)
        bad = list(ys); bad[n // 2] += 1
        put("ordinary/n%d_y+1" % n, c, t, x, bad)
        put("ordinary/n%d_x+1" % n, c, t, x + 1, ys)
        # x = 0 (inv(0) = 0: I' is its constant coefficient, x^np = 0) and x = 1
        c0 = valid_c(t, 0, ys)
        put("x_zero/n%d_valid" % n, c0, t, 0, ys)
        put("x_zero/n%d_t+1" % n, c0, t + 1, 0, ys)
        c1 = valid_c(t, 1, ys)
        put("x_one/n%d_valid" % n, c1, t, 1, ys)
        put("x_one/n%d_c+1" % n, c1 + 1, t, 1, ys)
    for n in (1, 8, 5):
        x, ys = rand_fr(rng), rand_ys(n)
        put("pi_inf/n%d_valid" % n, interp_at(ys, x, s), 0, x, ys)
        put("pi_inf/n%d_c+1" % n, interp_at(ys, x, s) + 1, 0, x, ys)
    # C == [I'(s)] G1: valid for any proof iff x^np == s^n, e.g. x = s w with w an n-th root of unity
    for n in (2, 8, 32):
        t, ys = rand_fr(rng), rand_ys(n)
        x = s * pow(root_of_unity(n), 1 + rng.randrange(n - 1), R) % R
        put("c_is_interp/n%d_x=sw" % n, interp_at(ys, x, s), t, x, ys)
        x = rand_fr(rng)
        put("c_is_interp/n%d_other_x" % n, interp_at(ys, x, s), t, x, ys)
    t, ys = rand_fr(rng), rand_ys(5)
    x = rand_fr(rng)
    put("c_is_interp/n5_other_x", interp_at(ys, x, s), t, x, ys)
    # the final addition doubles (C - I' == [x^np] pi): valid iff 2 x^np == s^n, which n = 1 reaches with x = s / 2
    t, ys = rand_fr(rng), rand_ys(1)
    x = s * inv(2) % R
    put("add_doubles/n1_x=s/2", interp_at(ys, x, s) + x * t, t, x, ys)
    for n in (8, 12):
        t, x, ys = rand_fr(rng), rand_fr(rng), rand_ys(n)
        put("add_doubles/n%d_other_x" % n, interp_at(ys, x, s) + pow(x, next_pow2(n), R) * t, t, x, ys)
    # ... cancels (C - I' == -[x^np] pi)
    for n in (2, 12):
        t, x, ys = rand_fr(rng), rand_fr(rng), rand_ys(n)
        put("add_cancels/n%d" % n, interp_at(ys, x, s) - pow(x, next_pow2(n), R) * t, t, x, ys)
    # the subtraction doubles: C == -[I'(s)] G1
    for n in (3, 8):
        x, ys = rand_fr(rng), rand_ys(n)
        c = -interp_at(ys, x, s) % R
        t = 2 * c * inv((pow(s, n, R) - pow(x, next_pow2(n), R)) % R) % R
        put("sub_doubles/n%d_valid" % n, c, t, x, ys)
        put("sub_doubles/n%d_t+1" % n, c, t + 1, x, ys)
    return rows
