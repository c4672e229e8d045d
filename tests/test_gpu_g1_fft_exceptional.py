"""Every device variant of the G1 transform on colliding and infinite operands (tests/g1_fft_cases.py crafts them, tests/test_g1_fft_cases.py
checks the crafting on the CPU): one stage launch of each of the 13 stage kernels, the direct passes on one, two and four lanes per term with
collisions at every level of their sum tree, and the public entry points at the batch sizes where the radix-2 network runs on four, two and one
lane per butterfly.  The hooks of go-kzg_amd/csrc/kzg_hip_internal.h force a variant per call and report the plan that ran; every test asserts
that plan, so a change of the dispatch cannot move a test off its kernel unnoticed.  Integer work: bit-exact against the C oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

import g1_fft_cases as gc
from oracle import koracle as ko

pytestmark = pytest.mark.gpu

SCALE = gc.STAGE_SCALE


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def fs(kz):
    fs = kz.FFTSettings(SCALE)
    yield fs
    fs.close()


def assert_points_equal(got, want):
    """bit-exact on the normalised images"""
    got, want = np.asarray(got).reshape(-1, 3, 6), np.asarray(want).reshape(-1, 3, 6)
    assert got.shape == want.shape
    bad = np.nonzero((got != ko.g1_affine(want)).any(axis=(1, 2)))[0]
    assert bad.size == 0, "first mismatching indices: %s" % bad[:8]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def by_size_plan(kz, fs, n, batch, m, dif=False):
    out = (C.c_uint32 * 5)()
    assert kz.lib().kzg_hip_test_g1_fft_plan(fs.h, n, batch, m, int(dif), out) == 0
    return tuple(out)


def run_stage(kz, fs, imgs, m, inverse, dif, lanes, mul=0):
    imgs = np.ascontiguousarray(imgs, dtype=np.uint64)
    out, plan = np.zeros_like(imgs), (C.c_uint32 * 3)()
    assert kz.lib().kzg_hip_test_g1_fft_stage(fs.h, _p(imgs), imgs.shape[1], imgs.shape[0], m, int(inverse), int(dif), lanes, mul, _p(out), plan) == 0
    return out, tuple(plan)


def run_direct(kz, fs, imgs, n, inverse, max_logr, lanes, n_out=0):
    imgs = np.ascontiguousarray(imgs, dtype=np.uint64)
    out = np.zeros((imgs.shape[0], n, 3, 6), dtype=np.uint64)
    assert kz.lib().kzg_hip_test_g1_fft_direct(fs.h, _p(imgs), n, imgs.shape[1], imgs.shape[0], int(inverse), max_logr, lanes, n_out, _p(out)) == 0
    return out


# ------------------------------------------------------------------ one stage, every variant
@functools.lru_cache(maxsize=None)
def stage_case(batch, m, inverse, dif):
    """the crafted state as images (batch rows tiled from at most 8 distinct ones) and the oracle's stage of it, butterfly by butterfly"""
    c = gc.StageCase(gc.STAGE_N, batch, m, inverse, dif)
    imgs = c.images()
    want = gc.oracle_stage(imgs[:c.nd], m, inverse, dif)
    return imgs, np.stack([want[b % c.nd] for b in range(batch)])


@pytest.mark.parametrize("inverse", [False, True], ids=["expanded", "reversed"])
@pytest.mark.parametrize("dif", [False, True], ids=["dit", "dif"])
@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("batch,m", gc.STAGE_SHAPES)
def test_one_stage_launch_of_every_variant_on_exceptional_butterflies(kz, fs, batch, m, lanes, dif, inverse):
    """x == +-w y (DIF: x == +-y), x / y / both infinite at j == 0 and j != 0, two images of one element and an affine operand at j == 0 -- in the first
    and last lane of a wavefront, in the last workgroup, in the first, middle and last row, between generic butterflies; 64 points in a scale-8 settings
    object (twiddle stride > 1)"""
    imgs, want = stage_case(batch, m, inverse, dif)
    got, plan = run_stage(kz, fs, imgs, m, inverse, dif, lanes)
    assert plan == gc.stage_plan(batch, m, lanes, dif), "batch %d, m %d, %d lanes no longer runs %s but %s" % (
        batch, m, lanes, gc.stage_variant(gc.stage_plan(batch, m, lanes, dif), dif), gc.stage_variant(plan, dif))
    assert_points_equal(got, want)


@pytest.mark.parametrize("dif", [False, True], ids=["dit", "dif"])
def test_forced_schedules_and_the_plan_by_size(kz, fs, dif):
    """what KZG_HIP_G1_MUL forces per process, per call: "regular" everywhere but the one-lane DIF stage (which has the NAF form only), "wnaf" on one
    lane whatever the shape and on several lanes only where every wavefront holds one twiddle; and these launches of at most 2048 butterflies are
    four lanes per butterfly by size"""
    imgs, want = stage_case(64, 2, False, dif)
    for lanes in (1, 2, 4):
        got, plan = run_stage(kz, fs, imgs, 2, False, dif, lanes, mul=1)
        assert plan == ((1, 1, 1) if (dif and lanes == 1) else (lanes, 0, 0))
        assert_points_equal(got, want)
    imgs, want = stage_case(3, 4, False, dif)
    for lanes in (1, 2, 4):
        got, plan = run_stage(kz, fs, imgs, 4, False, dif, lanes, mul=2)
        assert plan == ((1, 1, 0) if lanes == 1 else (lanes, 0, 0))
        assert_points_equal(got, want)
    for batch, m in gc.STAGE_SHAPES:
        assert by_size_plan(kz, fs, gc.STAGE_N, batch, m, dif)[:3] == gc.stage_plan(batch, m, 4, dif), (batch, m)
    got, plan = run_stage(kz, fs, imgs, 4, False, dif, 0)
    assert plan == gc.stage_plan(3, 4, 4, dif)
    assert_points_equal(got, want)


# ------------------------------------------------------------------ the direct passes
@functools.lru_cache(maxsize=None)
def direct_case(n, max_logr, rows, later, n_valid, inverse):
    c = gc.DirectCase(n, max_logr, inverse, rows, later, n_valid)
    imgs = c.images()
    ofs = ko.FFTSettings(SCALE)
    zero = ko.g1_zero(n - c.n_valid) if c.n_valid < n else np.zeros((0, 3, 6), dtype=np.uint64)
    return imgs, np.stack([ofs.fft_g1(np.concatenate([imgs[r], zero]), inverse) for r in range(rows)])


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("n,max_logr,rows,later,n_valid", gc.DIRECT_SHAPES)
def test_direct_passes_on_collisions_in_the_sum_tree(kz, fs, n, max_logr, rows, later, n_valid, lanes, inverse):
    """k_g1_fft_direct and k_g1_fft_direct_coop<2 / 4> at radix 16 and 8: in the first pass and (pulled back) in a later one, at every level of the tree,
    two terms or partial sums equal / opposite, an infinite partial sum meeting a finite one and the reverse, outputs whose terms are all infinite, with
    u == 0 and u != 0; the inverse transform multiplies the exponent-0 terms of its last pass too.  n_valid = 128: the pruned tree of the first pass"""
    imgs, want = direct_case(n, max_logr, rows, later, n_valid, inverse)
    assert_points_equal(run_direct(kz, fs, imgs, n, inverse, max_logr, lanes), want)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("max_logr", [4, 3])
def test_direct_passes_with_pruned_outputs(kz, fs, max_logr, lanes, inverse):
    """n_out = 128 of 256: the last pass computes the outputs u < 8 (radix 16) or u < 2 (8 . 8 . 4) only; the crafted outputs of that pass are among them"""
    n, lr, rows, later, n_valid = [s for s in gc.DIRECT_SHAPES if s[0] == 256 and s[1] == max_logr and s[4] is None][0]
    imgs, want = direct_case(n, lr, rows, later, n_valid, inverse)
    got = run_direct(kz, fs, imgs, n, inverse, max_logr, lanes, n_out=128)
    assert_points_equal(got[:, :128], want[:, :128])


# ------------------------------------------------------------------ through the public API, by size
@functools.lru_cache(maxsize=None)
def network_case(inverse):
    c = gc.NetworkCase(inverse)
    imgs = c.images()
    ofs = ko.FFTSettings(SCALE)
    return imgs, ko.g1_affine(np.stack([ofs.fft_g1(row, inverse) for row in imgs]).reshape(-1, 3, 6)).reshape(imgs.shape)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("batch,lanes", [(72, 4), (520, 2), (1032, 1)])
def test_fft_g1_batch_on_collisions_inside_the_network(kz, fs, batch, lanes, inverse):
    """fft_g1_batch on 64-point rows whose radix-2 network meets x == +-w y at j != 0 in stage m = 2, 8 or 32; 32 batch butterflies per stage: four lanes
    each up to 16384, two up to 32768, one above (on the 256 compute units of a whole device) -- the plans are asserted, stage by stage"""
    imgs, want = network_case(inverse)
    for m in (1, 2, 4, 8, 16, 32):
        plan = by_size_plan(kz, fs, 64, batch, m)
        assert plan[0] == lanes and plan[3] == 0, "64 points x %d rows, m = %d: plan %s" % (batch, m, plan)
    tile = np.arange(batch) % imgs.shape[0]
    assert_points_equal(fs.fft_g1_batch(imgs[tile], inverse), want[tile])


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_lone_fft_g1_on_collisions_in_its_direct_passes(kz, fs, inverse):
    """a lone crafted 256-point transform: by size two radix-16 passes on four lanes per term"""
    n, lr, rows, later, n_valid = gc.DIRECT_SHAPES[0]
    assert by_size_plan(kz, fs, n, 1, 1)[3:] == (4, 4)
    imgs, want = direct_case(n, lr, rows, later, n_valid, inverse)
    for r in (0, rows - 1):              # one row crafted in the first pass, one in the second
        assert_points_equal(fs.fft_g1(imgs[r], inverse), want[r])
