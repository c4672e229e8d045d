"""The shared-window table walk of large commitment batches (k_fb_digits, k_fb_accumulate_shared, k_fb_finish_shared in go-kzg_amd/csrc/k_msm.hip) and the
rule that decides which tables a KZGSettings handle holds (ensure_fixed_table / ensure_shared_table in capi_kzg.hip).

The table is T_s[i D + d - 1] = d P_i; a workgroup keeps one accumulator per window (Q = 64 // W quads of four lanes per window, the 4 Q lanes of a window
divide the workgroup's coefficients), and one quad per blob joins the W window sums by Horner's rule.  KZG_HIP_FB_SHARED_MIN_BATCH=1 sends every batch of
commit_to_poly_batch down that path, so the shapes here stay small: 256 points with signed 8-bit digits (W = 16, Q = 4) and 13-bit digits (W = 10, Q = 6,
four idle quads), and 4096 points with 16-bit digits (8 x 16 = 128 bits exactly: the top digit is the edge).

Every site that adds two points must survive equal and opposite operands, which random scalars never produce.  Two setups with a known secret make them
reachable with digit-sized scalars:
    secret 1  (every P_i = G):       two coefficients with the same digit hold the same table entry.  Where they meet depends on their positions: in one lane
                                     (its accumulator meets the entry it adds next, or its negative), in two lanes of a quad, in two quads of a window, in two
                                     workgroups of a blob (the Horner finish adds the partial sums of a window one after the other);
    secret 2  (P_i = 2^i G):         k_0 = 2^c puts G into window 1, k_c = +-1 puts +-2^c G into window 0: after its c doublings the Horner accumulator meets the
                                     next window sum or its negative.
Which site a PAIR of positions meets at depends on the launch shape (workgroups per blob follow the device's compute units), and shared_shape() / site() below only
restate that shape for a 256-CU device to NAME the sites.  Coverage does not rest on that model: the rows "256 equal terms" and "256 terms cancelling in pairs" put
equal (resp. opposite) operands on the first addition of EVERY site in every launch shape -- with one digit everywhere, the lanes of a quad, the quads of a window
and the workgroups of a blob all hold equal sums whenever they hold equally many coefficients, and a lane with two coefficients doubles at its second addition.
Expected values never come from MSM code of the library: the commitment of a row is [sum k_i s^i] G, one scalar multiplication of the oracle, and the first rows
of every batch are also compared with ko.lincomb_g1.  Outputs are normalised, so they must be byte-identical to the all-window walk (KZG_HIP_FB_LAYOUT=windows)."""
import os

import numpy as np
import pytest

from oracle import koracle as ko

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R = ko.R_MOD
LAMBDA = 0xac45a4010001a40200000000ffffffff
S_256 = 1927409816240961209460912649124
N = 256
FB_LANES = 131072            # lanes of one walk launch on 256 compute units (fb_blocks_per_blob): only the NAMES of the collision sites below depend on it


def shared_windows(c):
    return (128 + c - 1) // c


def shared_shape(n, batch, c):
    """(workgroups per blob, lanes per window) of k_fb_accumulate_shared, as launch_fb_msm_shared derives them on a 256-CU device"""
    w = shared_windows(c)
    lw = 4 * (64 // w)
    bpb = (FB_LANES // 256) // batch
    split = 1
    while split < 8 and batch * 2 * n * split * 2 <= FB_LANES:
        split *= 2
    bpb = max(1, min(bpb, (2 * n * split + 255) // 256, (n + lw - 1) // lw))
    return bpb, lw


def site(a, b, n, batch, c):
    """where the terms of coefficients a and b of a row first meet"""
    bpb, lw = shared_shape(n, batch, c)
    ga, gb = a // lw, b // lw                       # group g = t bpb + blk; lane a % lw
    if ga % bpb != gb % bpb:
        return "two workgroups (finish)"
    if a % lw == b % lw:
        return "one lane"
    if (a % lw) // 4 == (b % lw) // 4:
        return "two lanes of a quad"
    return "two quads of a window"


def row_of(entries, n=N):
    row = np.zeros((n, 4), dtype=np.uint64)
    idx = sorted(entries)
    row[idx] = ko.fr_from_ints([entries[i] % R for i in idx])
    return row


def want_point(dlog):
    dlog %= R
    return ko.g1_mul(ko.g1_generator(), ko.fr_from_ints([dlog])[0]) if dlog else ko.g1_zero(1)[0]


def affine(p):
    return ko.g1_affine(p).reshape(-1, 3, 6)


PAIR_AT = ((0, 1), (0, 2), (4, 7), (0, 4), (0, 12), (3, 23), (0, 16), (0, 24), (5, 53), (0, 48), (0, 96), (0, 112), (7, 119), (0, 128), (37, 165), (0, 255), (15, 240))


def secret1_rows(c):
    """(description, {index: scalar}) on the setup with every P_i = G"""
    rng = np.random.default_rng(c)
    D = 1 << (c - 1)
    out = []
    for a, b in PAIR_AT:
        for d in (1, D, D - 1, 3 << (2 * c), 1 << (c * (shared_windows(c) - 1))):      # window 0 (the largest digit: D), windows 2 and W - 1
            for sign in (1, -1):
                for phi in (False, True):
                    k = LAMBDA * d % R if phi else d                                      # lambda d splits into (0, d): the phi half alone
                    e = {a: sign * k % R, b: k}
                    out.append(("pair %d,%d d=%#x sign=%+d%s" % (a, b, d, sign, " phi" if phi else ""), dict(e)))
                    for extra in range(3):                                               # the walk goes on after the doubling / from infinity
                        e[int(rng.integers(0, N))] = int.from_bytes(rng.bytes(31), "little")
                    out.append(("pair %d,%d d=%#x sign=%+d%s in a dense row" % (a, b, d, sign, " phi" if phi else ""), e))
    out.append(("256 equal terms", {i: 5 for i in range(N)}))
    out.append(("256 terms cancelling in pairs", {i: (5 if i % 2 else R - 5) for i in range(N)}))
    out.append(("256 terms cancelling across halves of the row", {i: (D if i < 128 else R - D) for i in range(N)}))
    return out


def secret2_rows(c):
    """(description, {index: scalar}) on the setup P_i = 2^i G: the Horner accumulator, c doublings after window w + 1, meets window w"""
    out = []
    W = shared_windows(c)
    for w in (0, 1, W - 2):
        hi = 1 << (c * (w + 1))
        for last, what in ((1, "its double"), (R - 1, "its negative")):
            lo = (1 << (c * w)) if last == 1 else R - (1 << (c * w))
            out.append(("window %d of %d meets %s" % (w, W, what), {0: hi, c: lo}))
            out.append(("window %d of %d meets %s, more below" % (w, W, what), {0: hi, c: lo, 200: 12345}))
    # the same in the phi halves: lambda 2^(c (w + 1)) and +-lambda 2^(c w)
    out.append(("phi: window 0 meets its double", {0: LAMBDA * (1 << c) % R, c: LAMBDA}))
    out.append(("phi: window 0 meets its negative", {0: LAMBDA * (1 << c) % R, c: R - LAMBDA}))
    return out


EDGE = [0, 1, 2**14, 2**15, 2**16 - 1, 2**16, (1 << 255) % R, R - 1, R - 2**15, 0x8000800080008000, int("7fff" * 15, 16), int("8000" * 15, 16),
        LAMBDA, LAMBDA - 1, LAMBDA + 1, LAMBDA // 2, LAMBDA // 2 + 1, LAMBDA // 2 - 1, R - LAMBDA, R - LAMBDA // 2, R // 2, R // 2 + 1, (LAMBDA * (2**126 + 12345)) % R,
        (LAMBDA * int("7fff" * 7, 16) + int("8000" * 7, 16)) % R, (LAMBDA << 64) % R, 2**127 - 1, 2**127, 2**127 + 1, 2**128 - 1]


def test_crafted_rows_collide_as_intended():
    """CPU, oracle only: the setups are what the rows assume, and the two sums of a pair are equal or opposite points"""
    g = ko.g1_generator()
    ones = ko.generate_testing_setup_g1(1, 8)
    assert all(ko.g1_equal(p, g) for p in ones)
    twos = ko.generate_testing_setup_g1(2, 20)
    for c in (8, 13, 16):
        assert ko.g1_equal(ko.g1_mul(twos[0], ko.fr_from_ints([1 << c])[0]), twos[c])                       # G in window 1, c doublings later, is P_c in window 0
        assert ko.g1_equal(ko.g1_add(ko.g1_mul(twos[0], ko.fr_from_ints([1 << c])[0]), ko.g1_mul(twos[c], ko.fr_from_ints([R - 1])[0])), ko.g1_zero(1)[0])
    lam_g = ko.g1_mul(g, ko.fr_from_ints([LAMBDA])[0])
    assert ko.g1_equal(ko.g1_mul(ones[3], ko.fr_from_ints([LAMBDA * 77 % R])[0]), ko.g1_mul(lam_g, ko.fr_from_ints([77])[0]))
    # every collision site is named at least once at the batch sizes the GPU test runs
    for c in (8, 13):
        seen = {site(a, b, N, batch, c) for a, b in PAIR_AT for batch in (1, 3, 65, 130)}
        assert seen == {"two workgroups (finish)", "one lane", "two lanes of a quad", "two quads of a window"}, (c, seen)
    assert shared_shape(4096, 4096, 19) == (1, 36) and shared_shape(N, 130, 8) == (2, 16) and shared_shape(N, 65, 8) == (4, 16) and shared_shape(N, 1, 13) == (11, 24)


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def setups():
    return {"random": (S_256, ko.generate_testing_setup_g1(S_256, N)), "ones": (1, ko.generate_testing_setup_g1(1, N)), "twos": (2, ko.generate_testing_setup_g1(2, N))}


def dlog_of(entries, s):
    return sum(k * pow(s, i, R) for i, k in entries.items()) % R


def batches_of(rows, batch):
    """the rows in batches of `batch`, all-zero rows first, in the middle and last; the last batch is filled up with its own first rows"""
    zero_at = {0, batch // 2, batch - 1} if batch >= 5 else ({1} if batch >= 3 else set())
    out, cur = [], 0
    while cur < len(rows):
        picked = []
        for b in range(batch):
            if b in zero_at:
                picked.append(None)
            else:
                picked.append(cur % len(rows))
                cur += 1
        out.append(picked)
    return out


def expected(named, s):
    """(description, row, normalised commitment) of every crafted row: computed once, shared by all batch sizes"""
    return [(what, row_of(e), affine(want_point(dlog_of(e, s)))[0]) for what, e in named]


def check_rows(ks, crafted, batch, ref=None):
    named, rows, want = crafted, [r for _, r, _ in crafted], [w for _, _, w in crafted]
    inf = affine(ko.g1_zero(1))[0]
    for picked in batches_of(rows, batch):
        blobs = np.stack([rows[j] if j is not None else np.zeros((N, 4), dtype=np.uint64) for j in picked])
        got = np.asarray(ks.commit_to_poly_batch(blobs)).reshape(batch, 3, 6)
        for b, j in enumerate(picked):
            assert np.array_equal(got[b], inf if j is None else want[j]), "batch %d, row %d: %s" % (batch, b, "zero row" if j is None else named[j][0])
        if ref is not None:
            assert np.array_equal(got, np.asarray(ref(blobs)).reshape(batch, 3, 6))


@pytest.mark.gpu
@pytest.mark.parametrize("budget_gb,c", [(0.004, 8), (0.11, 13)])
def test_shared_walk_on_256_points(kz, setups, budget_gb, c, monkeypatch):
    monkeypatch.setenv("KZG_HIP_FB_SHARED_MIN_BATCH", "1")
    fs = kz.FFTSettings(8)
    made = []
    try:
        def settings(name, gb):
            ks = kz.KZGSettings(fs, setups[name][1])
            made.append(ks)
            ks.set_table_budget_gb(gb)
            return ks

        def windows_layout(ks_w):
            def run(blobs):
                with pytest.MonkeyPatch.context() as mp:
                    mp.setenv("KZG_HIP_FB_LAYOUT", "windows")
                    return ks_w.commit_to_poly_batch(blobs)
            return run

        # ---- random rows and the edge scalars against the oracle's LinCombG1 and the all-window walk of a second handle
        s, pts = setups["random"]
        ks, ks_w = settings("random", budget_gb), settings("random", 0.5)
        rng = np.random.default_rng(c)
        for batch in (1, 3, 65, 130):
            ints = [[int.from_bytes(rng.bytes(32), "little") % R for _ in range(N)] for _ in range(3)]
            ints[0][:len(EDGE)] = EDGE
            rows = [ints[b] if b < 3 else [v * (b + 1) % R for v in ints[b % 3]] for b in range(batch)]
            blobs = np.stack([ko.fr_from_ints(r) for r in rows])
            if batch >= 3:
                blobs[batch // 2] = 0
            got = np.asarray(ks.commit_to_poly_batch(blobs)).reshape(batch, 3, 6)
            assert ks.table_info()[:2] == (c, shared_windows(c)) and ks.table_additions() == 2 * shared_windows(c)
            for b in range(min(batch, 3)):
                assert np.array_equal(got[b], affine(ko.lincomb_g1(pts, blobs[b]))[0]), (batch, b)
            base = [ko.lincomb_g1(pts, ko.fr_from_ints(ints[b])) for b in range(3)]
            for b in range(batch):
                want = ko.g1_zero(1)[0] if batch >= 3 and b == batch // 2 else ko.g1_mul(base[b % 3], ko.fr_from_ints([b + 1 if b >= 3 else 1])[0])
                assert np.array_equal(got[b], affine(want)[0]), (batch, b)
            assert np.array_equal(got, np.asarray(windows_layout(ks_w)(blobs)).reshape(batch, 3, 6))
            assert ks_w.table_info()[0] == 11                                            # really another table
            ks.set_projective_outputs(True)
            proj = np.asarray(ks.commit_to_poly_batch(blobs)).reshape(batch, 3, 6)
            ks.set_projective_outputs(False)
            assert np.array_equal(affine(proj), got) and not np.array_equal(proj[0], got[0])
        # ---- every addition site on equal and opposite operands
        ks1, ks1_w = settings("ones", budget_gb), settings("ones", 0.5)
        rows1 = expected(secret1_rows(c), 1)
        for batch in (1, 3, 65, 130):
            check_rows(ks1, rows1 if batch >= 65 else rows1[::7], batch, windows_layout(ks1_w) if batch == 130 else None)
        assert ks1.table_info()[0] == c
        ks2 = settings("twos", budget_gb)
        rows2 = expected(secret2_rows(c), 2)
        for batch in (1, 65):
            check_rows(ks2, rows2, batch)
    finally:
        for k in made:
            k.close()
        fs.close()


@pytest.mark.gpu
def test_shared_walk_16_bit_digits_on_4096_points(kz, monkeypatch):
    """c = 16 on the 4096-point setup (12.9 GB): 8 windows of 16 bits are exactly 128 bits, the top digit takes the last carry; a short blob and two full ones"""
    monkeypatch.setenv("KZG_HIP_FB_SHARED_MIN_BATCH", "1")
    setup = ko.g1_decompress(np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1.bin"), "rb").read(), dtype=np.uint8))
    fs = kz.FFTSettings(12)
    ks = kz.KZGSettings(fs, setup)
    try:
        ks.set_table_budget_gb(13.0)
        full = np.stack([ko.synthetic_blob(40), ko.synthetic_blob(41)])
        full[0][:len(EDGE)] = ko.fr_from_ints(EDGE)
        full[1][4096 - len(EDGE):] = ko.fr_from_ints(EDGE)
        got = np.asarray(ks.commit_to_poly_batch(full)).reshape(2, 3, 6)
        assert ks.table_info() == (16, 8, 4096 * 32768 * 96) and ks.table_additions() == 16
        for b in range(2):
            assert np.array_equal(got[b], affine(ko.lincomb_g1(setup, full[b]))[0]), b
        short = np.stack([full[0][:1000], full[1][3096:], np.zeros((1000, 4), dtype=np.uint64)])
        got = np.asarray(ks.commit_to_poly_batch(short)).reshape(3, 3, 6)
        for b in range(3):
            assert np.array_equal(got[b], affine(ko.lincomb_g1(setup[:1000], short[b]))[0]), b
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("KZG_HIP_FB_LAYOUT", "windows")
            assert np.array_equal(np.asarray(ks.commit_to_poly_batch(short)).reshape(3, 3, 6), got)
    finally:
        ks.close()
        fs.close()


@pytest.mark.gpu
def test_table_rule(kz, setups, monkeypatch):
    """which tables a handle holds: one budget, small calls never evict the shared table, large calls replace the all-window table only for fewer additions"""
    monkeypatch.setenv("KZG_HIP_FB_SHARED_MIN_BATCH", "2")
    s, pts = setups["random"]
    rng = np.random.default_rng(5)
    blobs = np.stack([ko.fr_from_ints([int.from_bytes(rng.bytes(32), "little") % R for _ in range(N)]) for _ in range(3)])
    want = np.stack([affine(ko.lincomb_g1(pts, b))[0] for b in blobs])
    fs = kz.FFTSettings(8)
    win11 = (11, 12, 12 * N * 1024 * 96)

    def lone(ks, b=0):
        assert np.array_equal(np.asarray(ks.commit_to_poly(blobs[b])).reshape(3, 6), want[b])

    def large(ks):
        assert np.array_equal(np.asarray(ks.commit_to_poly_batch(blobs)).reshape(3, 3, 6), want)

    ks = kz.KZGSettings(fs, pts)
    try:
        # lone call, then large: the remainder (0.2 GB) holds 13-bit digits, 20 additions against 24 -- both tables stay
        ks.set_table_budget_gb(0.5)
        lone(ks)
        assert ks.table_info() == win11 and ks.table_additions() == 24
        large(ks)
        assert ks.table_info() == win11 and ks.table_additions() == 24
        lone(ks, 1); large(ks)
        assert ks.table_info() == win11
        # first call large: the shared table alone, from the whole budget (15-bit digits, 9 windows per half)
        ks.set_table_budget_gb(0.5)
        assert ks.table_info() == (0, 0, 0)
        large(ks)
        assert ks.table_info() == (15, 9, N * 16384 * 96) and ks.table_additions() == 18
        lone(ks, 2)                                                       # ... and the all-window table the remainder affords
        assert ks.table_info()[:2] == (9, 15) and ks.table_additions() == 30
        large(ks)
        assert ks.table_info()[:2] == (9, 15)
        # a budget that cannot hold both: 0.35 GB less the 0.30 GB all-window table leaves 24 additions, no better; the whole budget gives 20, so the
        # all-window table is replaced, later small calls get 10-bit windows from the remainder, and nothing changes any more
        ks.set_table_budget_gb(0.35)
        lone(ks)
        assert ks.table_info() == win11
        large(ks)
        assert ks.table_info() == (13, 10, N * 4096 * 96) and ks.table_additions() == 20
        for turn in range(2):
            lone(ks, turn)
            assert ks.table_info()[:2] == (10, 13) and ks.table_additions() == 26
            large(ks)
            assert ks.table_info()[:2] == (10, 13)
        # the layout switched off: large batches walk the all-window table and build nothing
        ks.set_table_budget_gb(0.5)
        monkeypatch.setenv("KZG_HIP_FB_LAYOUT", "windows")
        large(ks)
        assert ks.table_info() == win11
    finally:
        ks.close()
        fs.close()
