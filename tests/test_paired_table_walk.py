"""The paired-point table of large commitment batches (k_fb_build_paired_pass1, k_fb_digits_paired, k_fb_accumulate_paired in go-kzg_amd/csrc/k_msm.hip, the
index arithmetic of fb_pair_index.hpp) and its place in the rule that decides which tables a KZGSettings handle holds (capi_kzg.hip).

An entry is T_p[g E + idx(d0, d1)] = d0 P_2g + d1 P_2g+1 for signed c-bit digits; a window of the walk owns floor(256 / W) lanes, W = ceil(128 / c), and the block
end sums any lane count per window.  KZG_HIP_FB_LAYOUT=paired takes the widest digits of 10 .. 5 bits that the budget holds and KZG_HIP_FB_SHARED_MIN_BATCH=1
sends every batch down that path, so 256 points reach all of it: 5-bit digits (W = 26, 9 lanes per window), 7-bit digits (W = 19, 13 lanes) and the headline's
own 10-bit digits (W = 13, 19 lanes, 128 pairs of 525 312 entries).

What pairing adds to tests/test_shared_window_walk.py, whose helpers and row sets are imported: the table BUILD adds P_2g+1 along a run that starts at
d0 P_2g - D P_2g+1.  On the setups with secret 1 (every P_i = G) and secret r - 1 (P_i = (-1)^i G) the running point meets its addend, the negative of its addend
and infinity in every pair, and the table holds entries at infinity, which the walk must skip: the rows (d, -d) and (d, d) on one pair gather exactly those (on
one setup or the other), in window 0, a middle window and the top window, in the plain and in the phi half.  A half stays below 2^126.4, so the top window holds
what that leaves of d.  The two coefficients of a pair carry independent half signs (k and r - k').
Expected values come from one scalar multiplication of the oracle per row, [sum k_i s^i] G, and from ko.lincomb_g1; outputs are normalised, so they must be
byte-identical to the all-window walk of a second handle (KZG_HIP_FB_LAYOUT=windows)."""
import numpy as np
import pytest

from oracle import koracle as ko
import test_shared_window_walk as sw

R, N, LAMBDA, EDGE = sw.R, sw.N, sw.LAMBDA, sw.EDGE
affine = sw.affine


def paired_windows(c):
    return (128 + c - 1) // c


def paired_bytes(n, c):
    D = 1 << (c - 1)
    return ((n + 1) // 2) * 2 * D * (D + 1) * 96


def pair_rows(c):
    """(description, {index: scalar}): both digits of one pair's tuple set, the rest of the row empty or dense"""
    rng = np.random.default_rng(100 + c)
    D, W = 1 << (c - 1), paired_windows(c)
    top_cap = (LAMBDA // 2 - 1) >> (c * (W - 1))
    out, seen = [], set()
    for g in (0, 37, 127):
        for d in (1, D - 1, D):
            for w in (0, W // 2, W - 1):
                dd = min(d, top_cap) if w == W - 1 else d
                if (g, dd, w) in seen:
                    continue
                seen.add((g, dd, w))
                for sign, what in ((1, "(d, d)"), (-1, "(d, -d)")):
                    for phi in (False, True):
                        k = (dd << (c * w)) * (LAMBDA if phi else 1) % R
                        e = {2 * g: k, 2 * g + 1: sign * k % R}
                        name = "pair %d %s d=%d window %d%s" % (g, what, dd, w, " phi" if phi else "")
                        out.append((name, dict(e)))
                        if g == 37:
                            for extra in range(3):
                                e[int(rng.integers(0, N))] = int.from_bytes(rng.bytes(31), "little")
                            out.append((name + " in a dense row", e))
    for g in (0, 64, 127):                                  # independent half signs inside a pair: k splits as (+, .), r - k' as (-, .)
        k, k2 = int.from_bytes(rng.bytes(15), "little"), int.from_bytes(rng.bytes(15), "little")
        out.append(("pair %d: k and r - k'" % g, {2 * g: k, 2 * g + 1: R - k2}))
        out.append(("pair %d: r - k and k'" % g, {2 * g: R - k, 2 * g + 1: k2}))
        out.append(("pair %d: lambda k and r - lambda k'" % g, {2 * g: LAMBDA * k % R, 2 * g + 1: R - LAMBDA * k2 % R}))
        e = {2 * g: k, 2 * g + 1: R - k2}
        for extra in range(5):
            e[int(rng.integers(0, N))] = int.from_bytes(rng.bytes(32), "little") % R
        out.append(("pair %d: k and r - k' in a dense row" % g, e))
    return out


def test_pair_rows_gather_what_they_claim():
    """CPU, oracle only: on the two dependent setups the tuple of a pair row is the point at infinity on one of them"""
    g = ko.g1_generator()
    alt = ko.generate_testing_setup_g1(R - 1, 4)
    assert ko.g1_equal(alt[0], g) and ko.g1_equal(ko.g1_add(alt[0], alt[1]), ko.g1_zero(1)[0]) and ko.g1_equal(alt[2], g)
    for c in (5, 7, 10):
        rows = pair_rows(c)
        names = [n for n, _ in rows]
        assert len(set(names)) == len(names)
        lone = [(n, e) for n, e in rows if n.startswith("pair ") and " (d, " in n and "dense" not in n]
        assert len(lone) >= 3 * 4 * 7                       # three pairs, (d, +-d) x plain / phi, at least seven (d, window) sites each
        for n, e in lone:
            # d P_2g + (+-d) P_2g+1: secret 1 has P_2g+1 = P_2g, secret r - 1 has P_2g+1 = -P_2g -- (d, -d) is infinity on the first, (d, d) on the second
            on_ones, on_alt = sw.dlog_of(e, 1), sw.dlog_of(e, R - 1)
            assert (on_ones == 0) != (on_alt == 0), n
            assert (on_ones == 0) == ("(d, -d)" in n), n
    assert paired_bytes(4096, 10) == 103280541696 and paired_bytes(N, 10) + 12 * N * 1024 * 96 < 7e9 < paired_bytes(N, 10) + 11 * N * 2048 * 96


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def setups():
    return {"random": (sw.S_256, ko.generate_testing_setup_g1(sw.S_256, N)), "ones": (1, ko.generate_testing_setup_g1(1, N)),
            "alternating": (R - 1, ko.generate_testing_setup_g1(R - 1, N)), "twos": (2, ko.generate_testing_setup_g1(2, N))}


@pytest.mark.gpu
@pytest.mark.parametrize("budget_gb,c", [(0.01, 5), (0.2, 7), (7.0, 10)])
def test_paired_walk_on_256_points(kz, setups, budget_gb, c, monkeypatch):
    monkeypatch.setenv("KZG_HIP_FB_LAYOUT", "paired")
    monkeypatch.setenv("KZG_HIP_FB_SHARED_MIN_BATCH", "1")
    W = paired_windows(c)
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
            assert ks.table_info() == (c, W, paired_bytes(N, c)) and ks.table_additions() == W
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
        # ---- short rows: a last coefficient without a partner (n odd), one coefficient, one pair
        full = np.stack([ko.fr_from_ints(ints[b]) for b in range(3)])
        for n in (255, 1, 2):
            short = np.ascontiguousarray(full[:, :n])
            got = np.asarray(ks.commit_to_poly_batch(short)).reshape(3, 3, 6)
            for b in range(3):
                assert np.array_equal(got[b], affine(ko.lincomb_g1(pts[:n], short[b]))[0]), (n, b)
            assert np.array_equal(got, np.asarray(windows_layout(ks_w)(short)).reshape(3, 3, 6)), n
        ks.close(); made.remove(ks)
        # ---- dependent neighbours: the build meets addend = running point, its negative and infinity; the walk gathers entries at infinity
        pairs = pair_rows(c)
        for name in ("ones", "alternating"):
            sec = setups[name][0]
            ksd = settings(name, budget_gb)
            crafted = sw.expected(pairs, sec)
            for batch in (1, 65):
                sw.check_rows(ksd, crafted if batch == 65 else crafted[::5], batch)
            if name == "ones":
                # every addition site of the walk, the block end and the Horner finish on equal and opposite operands
                rows1 = sw.expected(sw.secret1_rows(c), 1)
                tail = rows1[-3:]                                                    # "256 equal terms", "cancelling in pairs", "across halves"
                ks1_w = settings("ones", 0.5)
                for batch in (1, 3, 65, 130):
                    sw.check_rows(ksd, rows1 if batch == 65 else rows1[::23] + tail, batch, windows_layout(ks1_w) if batch == 130 else None)
                ks1_w.close(); made.remove(ks1_w)
            assert ksd.table_info()[:2] == (c, W)
            ksd.close(); made.remove(ksd)
        ks2 = settings("twos", budget_gb)
        rows2 = sw.expected(sw.secret2_rows(c), 2)
        for batch in (1, 65):
            sw.check_rows(ks2, rows2, batch)
    finally:
        for k in made:
            k.close()
        fs.close()


@pytest.mark.gpu
def test_paired_table_rule(kz, setups, monkeypatch):
    """default mode: the paired table only at 10-bit digits and only for fewer additions than the single-point table of the same bytes"""
    monkeypatch.setenv("KZG_HIP_FB_SHARED_MIN_BATCH", "2")
    monkeypatch.delenv("KZG_HIP_FB_LAYOUT", raising=False)
    s, pts = setups["random"]
    rng = np.random.default_rng(6)
    blobs = np.stack([ko.fr_from_ints([int.from_bytes(rng.bytes(32), "little") % R for _ in range(N)]) for _ in range(3)])
    want = np.stack([affine(ko.lincomb_g1(pts, b))[0] for b in blobs])
    fs = kz.FFTSettings(8)

    def lone(ks, b=0):
        assert np.array_equal(np.asarray(ks.commit_to_poly(blobs[b])).reshape(3, 6), want[b])

    def large(ks):
        assert np.array_equal(np.asarray(ks.commit_to_poly_batch(blobs)).reshape(3, 3, 6), want)

    ks = kz.KZGSettings(fs, pts)
    try:
        # 0.5 GB hold paired 8-bit digits (16 additions against 18), narrower than the width that was measured: the single-point table, as before
        ks.set_table_budget_gb(0.5)
        large(ks)
        assert ks.table_info() == (15, 9, N * 16384 * 96) and ks.table_additions() == 18
        # 7 GB: paired 10-bit digits, 13 additions against the 14 of 19-bit single-point digits from the same bytes
        ks.set_table_budget_gb(7.0)
        assert ks.table_info() == (0, 0, 0)
        large(ks)
        assert ks.table_info() == (10, 13, paired_bytes(N, 10)) and ks.table_additions() == 13
        lone(ks, 1)                                                       # the all-window table the remainder (0.54 GB) affords; the paired table stays
        assert ks.table_info() == (11, 12, 12 * N * 1024 * 96) and ks.table_additions() == 24
        large(ks); lone(ks, 2); large(ks)
        assert ks.table_info()[:2] == (11, 12)
        # lone call first: the all-window table takes 6.4 GB (16 additions), the remainder holds nothing better, the whole budget 13: replaced
        ks.set_table_budget_gb(7.0)
        lone(ks)
        assert ks.table_info()[:2] == (16, 8) and ks.table_additions() == 16
        large(ks)
        assert ks.table_info() == (10, 13, paired_bytes(N, 10)) and ks.table_additions() == 13
        # the layouts of large batches switched off: the all-window table of the whole budget, nothing else is built
        ks.set_table_budget_gb(7.0)
        monkeypatch.setenv("KZG_HIP_FB_LAYOUT", "windows")
        large(ks)
        assert ks.table_info()[:2] == (16, 8) and ks.table_additions() == 16
    finally:
        ks.close()
        fs.close()
