"""The crafted-row generator (tests/verify_cases.py) itself: every class is there in both truth values, the exceptional relation a row is named
for really holds between its scalars, and the derived truth value agrees with the reference pairing on a sample of rows.  CPU only."""
import random

import pairing_ref as pr
import verify_cases as vc

R = vc.R
S = 1927409816240961209460912649124          # the testing setup's secret
S_ETH = 1337                                 # the fixture setup's


def by_class(rows):
    out = {}
    for row in rows:
        out.setdefault(row[0].split("/")[0], []).append(row)
    return out


def test_constants():
    assert R == pr.R
    assert (vc.LAMBDA * vc.LAMBDA + vc.LAMBDA + 1) % R == 0        # a primitive cube root of unity mod r: the eigenvalue of phi
    # the split restated here: k == +-|k1| +- k2 lambda, |k1| <= HL, k2 <= K2_MAX; the named edge scalars have the halves they are named for
    halves = {}
    for name, k in vc.edge_scalars():
        k1, k2, n1, n2 = vc.glv_split(k)
        assert ((-k1 if n1 else k1) + (-k2 if n2 else k2) * vc.LAMBDA) % R == k and k1 <= vc.HL and k2 <= vc.K2_MAX, name
        halves[name] = (k1, k2, n1, n2)
    assert halves["0"][:2] == (0, 0) and halves["1"][:2] == (1, 0) and halves["r-1"] == (1, 0, True, True)
    assert halves["lambda"][:2] == (0, 1) and halves["r-lambda"] == (0, 1, True, True) and halves["lambda-1"] == (1, 1, True, False)
    assert halves["k1_zero"][0] == 0 and halves["k1_zero"][1] > 2 ** 100
    assert halves["k2_zero_k1_max"] == (vc.HL, 0, False, False)
    assert halves["k1_min"] == (vc.HL, 1, True, False)
    assert halves["k2_max"][1] == vc.K2_MAX and halves["k2_max_neg"][1] == vc.K2_MAX and halves["k2_max_neg"][3]
    assert halves["both_max"][0] == vc.HL and halves["both_max"][1] >= vc.K2_MAX - 1 and halves["both_max_neg"][2:] == (True, True)
    assert halves["k2_max"][0] == 0 and halves["k2_max_k1_-1"] == (1, vc.K2_MAX, True, False)
    assert len({k for _, k in vc.edge_scalars()}) == len(vc.edge_scalars())


def test_single_rows_are_what_they_are_named():
    for s in (S, S_ETH):
        rows = vc.single_rows(s, random.Random(1))
        assert len({r[0] for r in rows}) == len(rows)                       # names are unique
        assert rows == vc.single_rows(s, random.Random(1))                   # and the generator is deterministic
        cls = by_class(rows)
        assert set(cls) == set(vc.SINGLE_CLASSES)
        for name, both in vc.SINGLE_CLASSES.items():
            wants = {r[5] for r in cls[name]}
            assert wants == ({True, False} if both else {False}), name
        edge = {k for _, k in vc.edge_scalars()}
        for name, c, t, x, y, want in rows:
            k = name.split("/")[0]
            assert all(0 <= v < R for v in (c, t, x, y))
            assert want == ((c - y + (x - s) * t) % R == 0), name
            if k == "ordinary":
                assert min(c, t, x, y).bit_length() > 200, name              # full width: both GLV halves of [x] pi and [y] G1
                assert min(vc.glv_split(x)[:2]) > 2 ** 100 and min(vc.glv_split(y)[:2]) > 2 ** 100, name
            elif k == "constant":
                assert t == 0 and want == (c == y), name
            elif k == "edge_x":
                assert x in edge and t != 0, name
            elif k == "edge_y":
                assert y in edge and t != 0, name
            elif k == "add_doubles":
                assert (c - y) % R == x * t % R and t != 0 and x != 0 and want == (2 * x % R == s % R), name
            elif k == "add_cancels":
                assert (c - y) % R == -x * t % R and t != 0 and x != 0 and not want, name
            elif k == "sub_doubles":
                assert (c + y) % R == 0 and c != 0 and t != 0, name
            elif k == "sub_cancels":
                assert c == y and t != 0 and want == (x == s % R), name
            elif k == "generator":
                assert c in (1, 2) and y in (1, 2) and t in (1, R - 1), name
        assert {x for n, _, _, x, _, _ in cls["edge_x"]} >= edge and {y for n, _, _, _, y, _ in cls["edge_y"]} >= edge
        assert any(r[3] == s * pow(2, -1, R) % R and r[5] for r in cls["add_doubles"])


def test_multi_rows_are_what_they_are_named():
    s = S
    rows = vc.multi_rows(s, random.Random(2))
    assert len({r[0] for r in rows}) == len(rows)
    cls = by_class(rows)
    assert set(cls) == set(vc.MULTI_CLASSES)
    for name, both in vc.MULTI_CLASSES.items():
        assert {r[6] for r in cls[name]} == ({True, False} if both else {False}), name
    for k in ("ordinary", "x_zero", "x_one"):                                # every length in both truth values, the non-powers of two included
        assert {(r[5], r[6]) for r in cls[k]} == {(n, w) for n in vc.MULTI_NS for w in (True, False)}, k
    assert {3, 5, 12} <= set(vc.MULTI_NS)
    for name, c, t, x, ys, n, want in rows:
        k = name.split("/")[0]
        npad = vc.next_pow2(n)
        assert len(ys) == n and npad >= n and npad & (npad - 1) == 0 and npad < 2 * n + 1
        i_s = vc.interp_at(ys, x, s)
        b, sn = pow(x, npad, R), pow(s, n, R)
        assert want == ((c - i_s + (b - sn) * t) % R == 0), name
        if k == "pi_inf":
            assert t == 0 and want == (c == i_s), name
        elif k == "c_is_interp":
            assert c == i_s and t != 0 and want == (b == sn), name
        elif k == "add_doubles":
            assert (c - i_s) % R == b * t % R and t != 0 and want == (2 * b % R == sn), name
        elif k == "add_cancels":
            assert (c - i_s) % R == -b * t % R and t != 0 and not want, name
        elif k == "sub_doubles":
            assert (c + i_s) % R == 0 and c != 0, name
        elif k == "x_zero":
            assert x == 0 and b == 0, name
        elif k == "x_one":
            assert x == 1, name
    assert any(r[6] and r[3] != s and pow(r[3], r[5], R) == pow(s, r[5], R) for r in cls["c_is_interp"])      # x = s w, w != 1


def test_interpolation_restated():
    # I' interpolates: with x = 1 and a power-of-two length it takes the values ys on the domain; with a coset shift x, I'(x w^j) = ys[j]
    rng = random.Random(3)
    for n in (1, 2, 8):
        ys = [rng.randrange(R) for _ in range(n)]
        w = vc.root_of_unity(n)
        for x in (1, rng.randrange(1, R)):
            for j in range(n):
                assert vc.interp_at(ys, x, x * pow(w, j, R) % R) == ys[j]
    # a length that is not a power of two is zero-padded: the same polynomial as the padded list, and x = 0 keeps the constant coefficient only
    ys = [rng.randrange(R) for _ in range(5)]
    at = rng.randrange(R)
    assert vc.interp_at(ys, 7, at) == vc.interp_at(ys + [0, 0, 0], 7, at)
    assert vc.interp_at(ys, 0, at) == sum(ys) * pow(8, -1, R) % R


def g1(k):
    return pr.g1_mul(pr.G1_GEN, k % R)


def g1_neg(Pt):
    return None if Pt is None else (Pt[0], -Pt[1] % pr.P)


def test_truth_values_agree_with_the_reference_pairing():
    """e(C - E, G2) == e(pi, [s^n - b] G2), the reference's arrangement (kzg_single_proofs.go:57-70, kzg_multi_proofs.go:47-75), on points made
    by the reference's double-and-add: one valid and one invalid row of each class whose rows differ in how the pairing inputs come about"""
    s = S % R
    rows = vc.single_rows(s, random.Random(1))
    picked = []
    for k in ("ordinary", "constant", "add_doubles", "add_cancels", "sub_doubles", "sub_cancels", "generator"):
        for w in (True, False):
            row = next((r for r in rows if r[0].startswith(k + "/") and r[5] == w), None)
            if row:
                picked.append(row)
    assert len(picked) == 13
    for name, c, t, x, y, want in picked:
        lhs = pr.g1_add(g1(c), g1_neg(g1(y)))
        got = pr.multi_pairing([(lhs, pr.G2_GEN), (g1_neg(g1(t)), pr.g2_mul(pr.G2_GEN, (s - x) % R))]) == pr.ONE12
        assert got == want, name
    mrows = vc.multi_rows(s, random.Random(2))
    for key in ("ordinary/n3_valid", "ordinary/n3_c+1", "ordinary/n12_valid", "c_is_interp/n8_x=sw", "c_is_interp/n8_other_x", "x_zero/n5_valid"):
        name, c, t, x, ys, n, want = next(r for r in mrows if r[0] == key)
        lhs = pr.g1_add(g1(c), g1_neg(g1(vc.interp_at(ys, x, s))))
        q = pr.g2_mul(pr.G2_GEN, (pow(s, n, R) - pow(x, vc.next_pow2(n), R)) % R)
        got = pr.multi_pairing([(lhs, pr.G2_GEN), (g1_neg(g1(t)), q)]) == pr.ONE12
        assert got == want, name
