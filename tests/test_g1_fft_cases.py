"""The case generator of the exceptional-operand tests of the G1 transform (tests/g1_fft_cases.py), checked without a GPU: its models of the
kernels' indexing reproduce oracle/pyref.py, a pulled-back input reproduces the chosen state, the C oracle's transform of the crafted POINTS is
the model times G, collisions show as the predicted infinities in the oracle's own output, and the generated inputs are what the GPU tests
(tests/test_gpu_g1_fft_exceptional.py) rely on: distinct and non-zero except where crafted, every class present, every placement taken."""
import random

import numpy as np
import pytest

import g1_fft_cases as gc
from oracle import koracle as ko
from oracle import pyref

R = gc.R
SCALE = gc.STAGE_SCALE
W = 1 << SCALE


def rand_vec(n, seed):
    rng = random.Random(seed)
    return [gc.rand_nz(rng) for _ in range(n)]


def assert_images_equal(got, want):
    assert np.array_equal(ko.g1_affine(got), ko.g1_affine(want))


def images_of(dlogs):
    return gc.points(dlogs, random.Random(5))


@pytest.fixture(scope="module")
def pfs():
    return pyref.FFTSettings(SCALE)


@pytest.fixture(scope="module")
def ofs():
    return ko.FFTSettings(SCALE)


# ------------------------------------------------------------------ the models against pyref
@pytest.mark.parametrize("inverse", [False, True])
def test_dit_and_dif_networks_equal_pyref(pfs, inverse):
    vals = rand_vec(64, 1)
    roots = gc.tables(SCALE)[inverse]
    want = pfs.fft(vals, inv=inverse)
    unscale = gc.inv(64) if inverse else 1
    assert [v * unscale % R for v in gc.dit_network(vals, roots, W)] == want
    state, m = list(vals), 32
    while m >= 1:                       # the DIF stages m = n / 2 ... 1 on natural order leave the result bit-reversed
        state = gc.dif_stage(state, m, roots, W)
        m //= 2
    assert [v * unscale % R for v in gc.bitrev(state)] == want


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n,max_logr", [(256, 4), (256, 3), (64, 4), (128, 4)])
def test_direct_passes_equal_pyref(pfs, n, max_logr, inverse):
    vals = rand_vec(n, 2)
    roots = gc.tables(SCALE)[inverse]
    assert gc.direct_transform(vals, max_logr, roots, W, inverse) == pfs.fft(vals, inv=inverse)


def test_pruned_first_pass_equals_the_full_one_on_padded_input():
    vals = rand_vec(128, 3) + [0] * 128
    roots = gc.tables(SCALE)[0]
    for logr, n_terms in ((4, 8), (3, 4)):
        assert gc.direct_pass(vals, logr, 1, roots, W, n_terms=n_terms) == gc.direct_pass(vals, logr, 1, roots, W)


@pytest.mark.parametrize("inverse", [False, True])
def test_pull_back_reproduces_the_state(inverse):
    roots = gc.tables(SCALE)[inverse]
    state = rand_vec(64, 4)
    for m in (2, 8, 32):
        assert gc.dit_network(gc.dit_pull_back(state, m, roots, W), roots, W, until=m) == state
    state = rand_vec(256, 5)
    for max_logr, p in ((4, 1), (3, 1), (3, 2)):
        assert gc.direct_transform(gc.direct_pull_back(state, p, max_logr, roots, W), max_logr, roots, W, inverse, until=p) == state


# ------------------------------------------------------------------ one stage
def stage_cases():
    return [gc.StageCase(gc.STAGE_N, batch, m, inverse, dif) for batch, m in gc.STAGE_SHAPES for inverse in (False, True) for dif in (False, True)]


def test_stage_cases_hold_every_class_at_every_placement():
    seen = set()
    for c in stage_cases():
        total = c.n // 2 * c.batch
        lanes = c.exceptional_lanes()
        classes_j0 = {cls for (d, g, j), cls in c.marks.items() if j == 0}
        classes_jn = {cls for (d, g, j), cls in c.marks.items() if j != 0}
        seen |= {(cls, 0) for cls in classes_j0} | {(cls, 1) for cls in classes_jn}
        if c.m > 1:
            assert classes_jn == set(gc.STAGE_CLASSES_ANY_J), (c.batch, c.m)
        if c.m < 32:
            assert classes_j0 == set(gc.STAGE_CLASSES_J0), (c.batch, c.m)
        # first and last lane of a wavefront whether a butterfly takes 1, 2 or 4 lanes; the last lane of the launch (last workgroup, last row)
        assert 0 in lanes and 63 in lanes and 64 in lanes and total - 1 in lanes
        rows = {gc.lane_to_butterfly(c.n, c.batch, c.m, t)[0] for t in lanes}
        assert {0, c.batch // 2, c.batch - 1} <= rows
        # generic lane neighbours: 16 consecutive butterflies share a wavefront even at four lanes each, and every such group holds a generic one
        for blk in {t // 16 for t in lanes}:
            assert len([t for t in lanes if t // 16 == blk]) < min(16, total - 16 * blk), (c.batch, c.m, blk)
        # the crafted relations hold on the discrete logs, and generic butterflies are generic
        for d in range(c.nd):
            row = c.distinct[d]
            for g, j, i0, i1 in gc.butterflies(c.n, c.m):
                w = 1 if c.dif else gc.twiddle(c.roots, W, c.m, j)
                x, wy = row[i0], w * row[i1] % R
                cls = c.marks.get((d, g, j))
                if cls in (None, "affine operand"):
                    assert x and wy and x != wy and (x + wy) % R, (d, g, j)
                else:
                    assert {"x==wy": x == wy != 0, "two images": x == wy != 0, "x==-wy": (x + wy) % R == 0 != x, "x inf": x == 0 != wy, "y inf": wy == 0 != x,
                            "both inf": x == 0 == wy}[cls], (d, g, j, cls)
    assert seen == {(cls, 0) for cls in gc.STAGE_CLASSES_J0} | {(cls, 1) for cls in gc.STAGE_CLASSES_ANY_J}


def test_stage_shapes_reach_all_thirteen_variants():
    """the plans the GPU test asserts, over its shapes and forced lanes: the three one-lane DIT kernels, the two one-lane DIF kernels, the eight quad / pair kernels"""
    got = {gc.stage_variant(gc.stage_plan(batch, m, lanes, dif), dif) for batch, m in gc.STAGE_SHAPES for lanes in (1, 2, 4) for dif in (False, True)}
    want = {"k_g1_fft_stage<0>", "k_g1_fft_stage<4, false>", "k_g1_fft_stage<4, true>", "k_g1_fft_stage_dif<false>", "k_g1_fft_stage_dif<true>"}
    want |= {"k_g1_fft_stage_quad<%s, %s, %d>" % (d, w, lanes) for d in ("true", "false") for w in ("true", "false") for lanes in (2, 4)}
    assert got == want and len(want) == 13
    # the one-lane DIT shapes: 96 butterflies on the regular schedule, NAF without rows, NAF with rows
    assert [gc.stage_plan(b, m, 1, False) for b, m in ((3, 4), (3, 32), (64, 32), (64, 2))] == [(1, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]


@pytest.mark.parametrize("dif", [False, True])
def test_stage_oracle_equals_model(dif):
    """the per-butterfly oracle of the GPU test on a crafted state == the model's discrete logs times G; "two images" are two images"""
    c = gc.StageCase(gc.STAGE_N, 3, 4, True, dif)
    imgs = c.images()
    got = gc.oracle_stage(imgs, c.m, c.inverse, dif)
    for b in range(c.batch):
        assert_images_equal(got[b], images_of(c.expected_dlogs(b)))
    (d, g, j), = [k for k, cls in c.marks.items() if cls == "two images"][:1]
    x, y = imgs[d, g * 2 * c.m + j], imgs[d, g * 2 * c.m + j + c.m]
    assert ko.g1_equal(x, y) and not np.array_equal(x, y)
    (d, i), = list(c.affine)[:1]
    assert np.array_equal(imgs[d, i], ko.g1_affine(imgs[d, i])[0])


@pytest.mark.parametrize("dif", [False, True])
def test_a_model_with_a_wrong_fallback_disagrees_with_the_oracle(dif):
    """sensitivity: a stage whose exceptional branch drops the sign of the difference is caught at the crafted butterflies, and only there"""
    c = gc.StageCase(gc.STAGE_N, 3, 4, False, dif)
    got = ko.g1_affine(gc.oracle_stage(c.images()[:1], c.m, c.inverse, dif)[0])
    wrong = (lambda x, y, w: ((x + y) % R, (y - x) * w % R)) if dif else (lambda x, wy: ((x + wy) % R, (wy - x) % R))
    bad = ko.g1_affine(images_of(c.expected_dlogs(0, on_collision=wrong)))
    differ = set(np.nonzero((got != bad).any(axis=(1, 2)))[0])
    crafted = {g * 2 * c.m + j + c.m for (d, g, j), cls in c.marks.items() if d == 0 and cls not in ("affine operand", "x==wy", "two images", "both inf")}
    assert differ and differ == crafted


# ------------------------------------------------------------------ the direct passes
@pytest.fixture(scope="module")
def direct_cases():
    return {(n, lr, nv, inverse): gc.DirectCase(n, lr, inverse, rows, later, nv) for n, lr, rows, later, nv in gc.DIRECT_SHAPES for inverse in (False, True)}


def test_direct_cases_craft_what_they_claim(direct_cases):
    seen = set()
    for key, c in direct_cases.items():
        for r, row in enumerate(c.rows):
            crafted_in_input = [m for m in c.marks if m[0] == r and m[1] == 0]
            if not crafted_in_input:            # pulled back from a later pass: pairwise distinct and non-zero
                assert 0 not in row and len(set(row)) == len(row), key
        for mark in c.marks:
            r, p, j, u, off, a, kind = mark
            levels = c.tree_of(mark)
            terms = levels[0]
            seen.add((p > 0, len(terms), off, kind, u != 0))
            if kind == "all inf":
                assert not any(terms)
                continue
            lane = levels[len(terms).bit_length() - 1 - off.bit_length()]      # the lane values at the entrance of level `off`
            assert len(lane) == 2 * off
            x, y = lane[a], lane[a + off]
            assert {"equal": x == y != 0, "opposite": (x + y) % R == 0 != x, "inf meets finite": x == 0 != y, "finite meets inf": y == 0 != x}[kind], (key, mark)
            if 2 * off < len(terms) and kind in ("equal", "opposite"):      # partial sums collide while all terms differ, also up to sign
                assert 0 not in terms and len({t for t in terms} | {-t % R for t in terms}) == 2 * len(terms), (key, mark)
    for later, n_terms in ((False, 16), (True, 16), (False, 8), (True, 8), (True, 4)):
        offs, o = [], n_terms // 2
        while o:
            offs.append(o)
            o //= 2
        for off in offs:
            for kind in gc.TREE_KINDS:
                assert {(later, n_terms, off, kind, False), (later, n_terms, off, kind, True)} & seen, (later, n_terms, off, kind)
        assert {(later, n_terms, 0, "all inf", False), (later, n_terms, 0, "all inf", True)} & seen
    assert {s[4] for s in seen if not s[0]} == {False, True} and {s[4] for s in seen if s[0]} == {False, True}      # u == 0 and u != 0, first and later pass


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n,max_logr,n_valid", [(64, 4, None), (64, 3, None), (256, 3, 128)])
def test_direct_oracle_equals_model(ofs, direct_cases, n, max_logr, n_valid, inverse):
    c = direct_cases[(n, max_logr, n_valid, inverse)]
    imgs = c.images()
    zero = ko.g1_zero(n - c.n_valid) if c.n_valid < n else np.zeros((0, 3, 6), dtype=np.uint64)
    for r in range(len(c.rows)):
        got = ofs.fft_g1(np.concatenate([imgs[r], zero]), inverse)
        want = c.expected_dlogs(r)
        assert_images_equal(got, images_of(want))
        # opposite partial sums at the last level of the last pass: the predicted infinity in the oracle's own output
        ns = 1 << sum(c.radices[:-1])
        for (rr, p, j, u, off, a, kind) in c.marks:
            if rr == r and p + 1 == len(c.radices) and ((off == 1 and kind == "opposite") or kind == "all inf"):
                idx = gc.direct_out_index(n, c.radices[-1], ns, j, u)
                assert want[idx] == 0 and not ko.g1_affine(got)[idx, 2].any()


def test_one_crafted_256_point_row_through_the_oracle(ofs, direct_cases):
    c = direct_cases[(256, 4, None, False)]
    assert_images_equal(ofs.fft_g1(c.images()[3]), images_of(c.expected_dlogs(3)))


# ------------------------------------------------------------------ the whole network
@pytest.mark.parametrize("inverse", [False, True])
def test_network_rows_are_distinct_and_show_their_collisions(ofs, inverse):
    c = gc.NetworkCase(inverse)
    imgs = c.images()
    assert {m for (_, m, _, _, _) in c.marks} == set(gc.NETWORK_STAGES)
    assert {cls for (_, _, _, _, cls) in c.marks} == {"x==wy", "x==-wy"}
    for d, row in enumerate(c.rows):
        assert 0 not in row and len(set(row)) == len(row)
        mine = [mk for mk in c.marks if mk[0] == d]
        m = mine[0][1]
        state = gc.dit_network(row, c.roots, W, until=m)
        for (_, _, g, j, cls) in mine:
            assert j != 0
            x, wy = state[g * 2 * m + j], gc.twiddle(c.roots, W, m, j) * state[g * 2 * m + j + m] % R
            assert {"x==wy": x == wy != 0, "x==-wy": (x + wy) % R == 0 != x}[cls]
        got = ofs.fft_g1(imgs[d], inverse)
        want = c.expected_dlogs(d)
        assert_images_equal(got, images_of(want))
        if m == 32:         # a collision in the last stage is an infinite output: x == w y at its second index, x == -w y at its first
            for (_, _, g, j, cls) in mine:
                if cls in ("x==wy", "x==-wy"):
                    idx = j + (32 if cls == "x==wy" else 0)
                    assert want[idx] == 0 and not ko.g1_affine(got)[idx, 2].any()
