"""Crafted inputs for the G1 transform kernels: operands that collide (P == +-Q) or are infinite exactly where a kernel's fast path has to
decline -- at a chosen butterfly of a chosen radix-2 stage, or at a chosen level of the sum tree of a chosen direct pass.

Everything is done on discrete logarithms: a point is a G, so every intermediate value of a transform is a number mod r (0 = infinity) and
each stage / pass is an invertible linear map on F_r^n.  The models below restate the kernels' INDEXING (k_g1_fft_stage, k_g1_fft_stage_dif,
k_g1_fft_direct in go-kzg_amd/csrc/k_g1.hip) in plain Python; a state chosen at the entrance of any stage or pass is pulled back to an input
vector by inverting the earlier ones.  tests/test_g1_fft_cases.py checks the models against oracle/pyref.py and the C oracle on the CPU;
tests/test_gpu_g1_fft_exceptional.py feeds the cases to the device.  A plain helper module, imported by name."""
import random

import numpy as np

from oracle import koracle as ko
from oracle import pyref

R = pyref.R
P = pyref.P


def inv(a):
    return pow(a, -1, R)


def rev_bits(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def tables(scale):
    """(expanded, reversed) root tables of a settings object of width 2^scale, W + 1 entries each (fft.go:21-54)"""
    fs = pyref.FFTSettings(scale)
    return fs.expanded, fs.reversed


# ---------------------------------------------------------------------------------------------- (a), (b): the radix-2 stages
def butterflies(n, m):
    """(g, j, i0, i1) of the stage of half-size m, as the kernels index them"""
    for g in range(n // 2 // m):
        for j in range(m):
            i0 = g * 2 * m + j
            yield g, j, i0, i0 + m


def twiddle(roots, W, m, j):
    return roots[j * (W // (2 * m))]


def dit_stage(state, m, roots, W, on_collision=None):
    """(x, y) -> (x + w y, x - w y); on_collision(x, wy) replaces the result where x == +-w y or an operand is infinite (sensitivity check)"""
    out = list(state)
    for g, j, i0, i1 in butterflies(len(state), m):
        x, wy = state[i0], twiddle(roots, W, m, j) * state[i1] % R
        exceptional = x == 0 or wy == 0 or x == wy or (x + wy) % R == 0
        out[i0], out[i1] = on_collision(x, wy) if (exceptional and on_collision) else ((x + wy) % R, (x - wy) % R)
    return out


def dit_stage_inverse(state, m, roots, W):
    out = list(state)
    i2 = inv(2)
    for g, j, i0, i1 in butterflies(len(state), m):
        a, b = state[i0], state[i1]
        out[i0], out[i1] = (a + b) * i2 % R, (a - b) * i2 % R * inv(twiddle(roots, W, m, j)) % R
    return out


def dif_stage(state, m, roots, W, on_collision=None):
    """(x, y) -> (x + y, (x - y) w)"""
    out = list(state)
    for g, j, i0, i1 in butterflies(len(state), m):
        x, y, w = state[i0], state[i1], twiddle(roots, W, m, j)
        exceptional = x == 0 or y == 0 or x == y or (x + y) % R == 0
        out[i0], out[i1] = on_collision(x, y, w) if (exceptional and on_collision) else ((x + y) % R, (x - y) * w % R)
    return out


def bitrev(vals):
    bits = (len(vals) - 1).bit_length()
    return [vals[rev_bits(i, bits)] for i in range(len(vals))]


def dit_network(vals, roots, W, until=None):
    """bit reversal, then the stages m = 1, 2, ... (all of them, or those below `until`): the state at the entrance of stage `until`"""
    state, m = bitrev(vals), 1
    while m < len(vals) and m != until:
        state = dit_stage(state, m, roots, W)
        m *= 2
    return state


def dit_pull_back(state, m, roots, W):
    """the input vector whose state at the entrance of stage m is `state`"""
    while m > 1:
        m //= 2
        state = dit_stage_inverse(state, m, roots, W)
    return bitrev(state)


# ---------------------------------------------------------------------------------------------- (c): the direct passes
def direct_radices(n, max_logr):
    """log2 of the radix of each pass: max_logr while that many bits are left, then the rest (launch_g1_fft_direct)"""
    left, out = n.bit_length() - 1, []
    while left:
        out.append(min(max_logr, left))
        left -= out[-1]
    return out


def direct_coefficient(n, logr, ns, j, u, t, roots, W, scale=1):
    """what term t of output (j, u) multiplies in[j + t n / R] by"""
    cols = n >> logr
    e = (t * (cols // ns) * (ns * u + j % ns)) % n
    return roots[e * (W // n)] * scale % R


def direct_out_index(n, logr, ns, j, u):
    k = j % ns
    return (j - k) * (1 << logr) + k + u * ns


def direct_pass(state, logr, ns, roots, W, scale=1, n_terms=None):
    """out[(j - k) R + k + u Ns] = the halving tree over w^(t (n / (Ns R)) (Ns u + k)) in[j + t n / R], t < n_terms"""
    n, rr = len(state), 1 << logr
    cols = n >> logr
    out = [0] * n
    for j in range(cols):
        for u in range(rr):
            terms = [direct_coefficient(n, logr, ns, j, u, t, roots, W, scale) * state[j + t * cols] % R for t in range(n_terms or rr)]
            out[direct_out_index(n, logr, ns, j, u)] = tree_levels(terms)[-1][0]
    return out


def tree_levels(terms):
    """the lane values at the entrance of every level of the sum tree (lane tt adds lane tt + off, off = T / 2 ... 1) and, last, the sum"""
    levels = [list(terms)]
    off = len(terms) // 2
    while off >= 1:
        cur = levels[-1]
        levels.append([(cur[tt] + cur[tt + off]) % R for tt in range(off)])
        off //= 2
    return levels


def direct_pass_inverse(state, logr, ns, roots, W, scale=1):
    """a pass is, per column j, a size-R transform of the twisted inputs: undo both"""
    n, rr = len(state), 1 << logr
    cols = n >> logr
    out = [0] * n
    ir = inv(rr)
    for j in range(cols):
        outs = [state[direct_out_index(n, logr, ns, j, u)] for u in range(rr)]
        omega_inv = inv(roots[(cols % n) * (W // n)])           # w^(n / R): out_u = sum_t omega^(t u) * (w^(t c k) in_t)
        for t in range(rr):
            tw = ir * sum(pow(omega_inv, t * u, R) * outs[u] for u in range(rr)) % R
            out[j + t * cols] = tw * inv(direct_coefficient(n, logr, ns, j, 0, t, roots, W, scale)) % R
    return out


def direct_transform(vals, max_logr, roots, W, inverse=False, until=None):
    """the passes in order (all, or those before pass `until`); the 1 / n of the inverse transform rides on the last pass"""
    state, ns = list(vals), 1
    radices = direct_radices(len(vals), max_logr)
    for p, logr in enumerate(radices):
        if p == until:
            break
        state = direct_pass(state, logr, ns, roots, W, inv(len(vals)) if (inverse and p + 1 == len(radices)) else 1)
        ns <<= logr
    return state


def direct_pull_back(state, p, max_logr, roots, W):
    """the input vector whose state at the entrance of pass p (not the one after the last) is `state`"""
    radices = direct_radices(len(state), max_logr)
    ns = [1 << sum(radices[:q]) for q in range(len(radices))]
    for q in range(p - 1, -1, -1):
        state = direct_pass_inverse(state, radices[q], ns[q], roots, W)
    return state


# ---------------------------------------------------------------------------------------------- points
def u64s(v):
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]


def rescale(img, z):
    """the Kilic image of the same point with its Jacobian Z multiplied by z"""
    X, Y, Z = (sum(int(row[i]) << (64 * i) for i in range(6)) for row in np.asarray(img).reshape(3, 6))
    return np.array([u64s(X * z * z % P), u64s(Y * z * z * z % P), u64s(Z * z % P)], dtype=np.uint64)


_POINTS = {}


def point(a, z=None):
    """a G from the oracle: normalised (z None), or the Jacobian image with Z = z; a == 0: infinity"""
    a %= R
    if a == 0:
        return ko.g1_zero(1)[0]
    if a not in _POINTS:
        _POINTS[a] = ko.g1_affine(ko.g1_mul(ko.g1_generator(), ko.fr_from_ints([a])[0]))[0]
    return _POINTS[a] if z is None else rescale(_POINTS[a], z)


def points(dlogs, rng, affine=()):
    """images of a vector of discrete logs, each with a random Jacobian Z except the positions in `affine` (Z = 1)"""
    return np.stack([point(a, None if i in affine else rng.randrange(2, P)) for i, a in enumerate(dlogs)])


def rand_nz(rng):
    return rng.randrange(1, R)


# ---------------------------------------------------------------------------------------------- one stage, every variant
STAGE_CLASSES_ANY_J = ("x==wy", "x==-wy", "x inf", "y inf", "both inf")          # for DIF read w as 1: x == y, x == -y
STAGE_CLASSES_J0 = STAGE_CLASSES_ANY_J + ("two images", "affine operand")
# (batch, m): regular schedule at 96 butterflies (a partly filled last workgroup), NAF without digit rows (m = 32: one butterfly with j == 0 per row;
# m = 16: two, enough for every class at j == 0) and with them, j == 0 only
STAGE_SHAPES = ((3, 4), (3, 32), (64, 32), (64, 16), (64, 2), (3, 1), (64, 1))
STAGE_N = 64
STAGE_SCALE = 8          # twiddle stride W / (2m) = 2 ... 128: never 1
MAX_DISTINCT_ROWS = 8


def stage_plan(batch, m, lanes, dif, n=STAGE_N):
    """(lanes, width-5 NAF schedule, digits from precomputed rows) the library must run for a stage launch with `lanes` forced, restated from the
    rules of g1_fft_stage_plan (k_g1.hip): the GPU tests compare the plan the hook returns with this, so a shape that no longer gives its variant fails"""
    per_twiddle = n // 2 // m * batch
    if lanes > 1:
        wnaf = per_twiddle * lanes % 64 == 0
        return lanes, int(wnaf), int(wnaf)
    wnaf = dif or per_twiddle % 64 == 0 or per_twiddle >= 256
    return 1, int(wnaf), int(wnaf and per_twiddle >= 512)


# the device variants of a stage, named as the kernels are instantiated
def stage_variant(plan, dif):
    lanes, wnaf, rows = plan
    if lanes > 1:
        return "k_g1_fft_stage_quad<%s, %s, %d>" % ("true" if dif else "false", "true" if wnaf else "false", lanes)
    if dif:
        return "k_g1_fft_stage_dif<%s>" % ("true" if rows else "false")
    return "k_g1_fft_stage<4, %s>" % ("true" if rows else "false") if wnaf else "k_g1_fft_stage<0>"


def lane_to_butterfly(n, batch, m, t):
    """lane t of a stage launch -> (row, g, j): twiddle-major order"""
    groups = n // 2 // m
    j, rem = divmod(t, groups * batch)
    b, g = divmod(rem, groups)
    return b, g, j


def butterfly_to_lane(n, batch, m, b, g, j):
    groups = n // 2 // m
    return j * groups * batch + b * groups + g


class StageCase:
    """rows: batch x n discrete logs of the stage's input state (row b is distinct row b % len(distinct)); marks: {(d, g, j): class} of the
    exceptional butterflies of distinct row d; affine: positions (d, i) whose image has Z = 1; same: (d, g) whose x and y are one group element"""

    def __init__(self, n, batch, m, inverse, dif, scale=STAGE_SCALE, seed=0):
        self.n, self.batch, self.m, self.inverse, self.dif, self.W = n, batch, m, inverse, dif, 1 << scale
        expanded, reverse = tables(scale)
        self.roots = reverse if inverse else expanded
        rng = random.Random("stage %d %d %d %d %d %d" % (n, batch, m, inverse, dif, seed))
        self.nd = min(batch, MAX_DISTINCT_ROWS)
        self.distinct = [[rand_nz(rng) for _ in range(n)] for _ in range(self.nd)]
        self.marks, self.affine = {}, set()
        total = n // 2 * batch
        # the lanes that must be exceptional: first and last lane of a wavefront for 1, 2 and 4 lanes per butterfly (t = 0 and 64; t = 63),
        # the last lane of the launch (last workgroup, last row), one in the middle row
        forced = [0, 63, 64, total - 1, butterfly_to_lane(n, batch, m, batch // 2, 0, m - 1)]
        slots = []
        for t in forced:
            if 0 <= t < total:
                b, g, j = lane_to_butterfly(n, batch, m, t)
                if (b % self.nd, g, j) not in slots:
                    slots.append((b % self.nd, g, j))
        # ... and every other butterfly of each kind (j == 0, j != 0) of every distinct row, shifted by the row: generic lane neighbours everywhere
        for d in range(self.nd):
            for kind in (0, 1):
                own = [(d, g, j) for g, j, _, _ in butterflies(n, m) if (j != 0) == bool(kind)]
                own.sort(key=lambda s: butterfly_to_lane(n, batch, m, s[0], s[1], s[2]))
                slots += [s for s in own[d % 2::2] if s not in slots]
        turn = {0: 0, 1: 0}
        for d, g, j in slots:
            classes = STAGE_CLASSES_J0 if j == 0 else STAGE_CLASSES_ANY_J
            cls = classes[turn[j != 0] % len(classes)]
            turn[j != 0] += 1
            self._place(rng, d, g, j, cls)

    def _place(self, rng, d, g, j, cls):
        row, i0 = self.distinct[d], g * 2 * self.m + j
        i1 = i0 + self.m
        w = 1 if self.dif else twiddle(self.roots, self.W, self.m, j)
        y = rand_nz(rng)
        if cls in ("x==wy", "two images"):
            row[i0], row[i1] = w * y % R, y
        elif cls == "x==-wy":
            row[i0], row[i1] = -w * y % R, y
        elif cls == "x inf":
            row[i0] = 0
        elif cls == "y inf":
            row[i1] = 0
        elif cls == "both inf":
            row[i0] = row[i1] = 0
        elif cls == "affine operand":
            self.affine.add((d, i1 if (g + d) % 2 else i0))
        self.marks[(d, g, j)] = cls

    def row_dlogs(self, b):
        return self.distinct[b % self.nd]

    def images(self):
        """batch x n x 3 x 6: every point with a random Jacobian Z of its own (so "two images" are two), Z = 1 at the affine positions"""
        rng = random.Random("images %d %d %d" % (self.batch, self.m, self.inverse))
        rows = [points(row, rng, {i for (dd, i) in self.affine if dd == d}) for d, row in enumerate(self.distinct)]
        return np.stack([rows[b % self.nd] for b in range(self.batch)])

    def expected_dlogs(self, b, on_collision=None):
        stage = dif_stage if self.dif else dit_stage
        return stage(self.row_dlogs(b), self.m, self.roots, self.W, on_collision)

    def exceptional_lanes(self):
        return sorted(butterfly_to_lane(self.n, self.batch, self.m, b, g, j) for b in range(self.batch) for (d, g, j) in self.marks if d == b % self.nd)


def oracle_stage(imgs, m, inverse, dif, scale=STAGE_SCALE):
    """one stage on rows of point images by the oracle's group operations, butterfly by butterfly: (x + w y, x - w y) or (x + y, (x - y) w)"""
    ofs = ko.FFTSettings(scale)
    roots, W = (ofs.reverse_roots() if inverse else ofs.expanded_roots()), 1 << scale
    out = np.array(imgs, copy=True)
    for r in range(imgs.shape[0]):
        for g, j, i0, i1 in butterflies(imgs.shape[1], m):
            x, y, w = imgs[r, i0], imgs[r, i1], roots[j * (W // (2 * m))]
            if dif:
                out[r, i0], out[r, i1] = ko.g1_add(x, y), ko.g1_mul(ko.g1_sub(x, y), w)
            else:
                wy = ko.g1_mul(y, w)
                out[r, i0], out[r, i1] = ko.g1_add(x, wy), ko.g1_sub(x, wy)
    return out


# ---------------------------------------------------------------------------------------------- the direct passes
TREE_KINDS = ("equal", "opposite", "inf meets finite", "finite meets inf")


class DirectCase:
    """`rows` input rows (discrete logs, n_valid each) for the direct passes of radix 2^max_logr.  The first half of the rows is crafted in pass 0
    (directly on the input), the second half in pass `later` (a state at its entrance, pulled back).  Every column j of a crafted pass carries one
    crafted output (j, u): at level `off` of its sum tree lane a meets lane a + off with the two partial sums equal, opposite, the first infinite
    or the second infinite (at off = T / 2 the partial sums are single terms); or ALL its terms are infinite.  marks: [(row, pass, j, u, off, a, kind)]"""

    def __init__(self, n, max_logr, inverse, rows, later, n_valid=None, scale=STAGE_SCALE, seed=0):
        self.n, self.max_logr, self.inverse, self.later, self.W = n, max_logr, inverse, later, 1 << scale
        self.n_valid = n_valid or n
        expanded, reverse = tables(scale)
        self.roots = reverse if inverse else expanded
        self.radices = direct_radices(n, max_logr)
        rng = random.Random("direct %d %d %d %d %d %d" % (n, max_logr, inverse, rows, self.n_valid, seed))
        self.marks, self.rows = [], []
        turn = {0: 0, later: 0}
        for r in range(rows):
            p = 0 if (r < (rows + 1) // 2 or later is None) else later
            state = [rand_nz(rng) if i < self.n_valid or p else 0 for i in range(n)]
            turn[p] = self._craft(rng, r, p, state, turn[p])
            vals = direct_pull_back(state, p, max_logr, self.roots, self.W)
            assert p or all(v == 0 for v in vals[self.n_valid:])
            self.rows.append(vals[:self.n_valid])

    def pass_shape(self, p):
        logr = self.radices[p]
        ns = 1 << sum(self.radices[:p])
        cols = self.n >> logr
        n_terms = 1 << logr
        if p == 0:
            while n_terms > 1 and cols * (n_terms // 2) >= self.n_valid:      # terms beyond the valid input are infinite: the pruned tree
                n_terms //= 2
        scale = inv(self.n) if (self.inverse and p + 1 == len(self.radices)) else 1
        return logr, ns, cols, n_terms, scale

    def specs(self, n_terms):
        out, off = [], n_terms // 2
        while off >= 1:
            out += [(off, kind) for kind in TREE_KINDS]
            off //= 2
        return out + [(0, "all inf")]

    def _craft(self, rng, r, p, state, turn):
        logr, ns, cols, n_terms, scale = self.pass_shape(p)
        specs = self.specs(n_terms)
        last = p + 1 == len(self.radices)
        for j in range(cols):
            off, kind = specs[turn % len(specs)]
            # u == 0 (no multiplication in pass 0) and u != 0 alternate per spec; of the last pass only small u, so that pruned outputs keep them
            u = 0 if (turn // len(specs) + turn) % 2 == 0 else (1 if last else rng.randrange(1, 1 << logr))
            turn += 1
            if kind == "all inf":
                for t in range(1 << logr):
                    state[j + t * cols] = 0
                self.marks.append((r, p, j, u, 0, 0, kind))
                continue
            a = rng.randrange(off)
            coef = [direct_coefficient(self.n, logr, ns, j, u, t, self.roots, self.W, scale) for t in range(n_terms)]
            terms = [coef[t] * state[j + t * cols] % R for t in range(n_terms)]
            # lane x of level `off` holds the sum of the terms t = x mod 2 off; its lowest term is t = x: move that one
            lane = lambda x: sum(terms[t] for t in range(x, n_terms, 2 * off)) % R
            if kind == "equal":
                terms[a + off] = (terms[a + off] + lane(a) - lane(a + off)) % R
            elif kind == "opposite":
                terms[a + off] = (terms[a + off] - lane(a) - lane(a + off)) % R
            elif kind == "inf meets finite":
                terms[a] = (terms[a] - lane(a)) % R
            else:
                terms[a + off] = (terms[a + off] - lane(a + off)) % R
            for t in (a, a + off):
                state[j + t * cols] = terms[t] * inv(coef[t]) % R
            self.marks.append((r, p, j, u, off, a, kind))
        return turn

    def images(self):
        rng = random.Random("direct images %d %d %d" % (self.n, self.max_logr, self.inverse))
        return np.stack([points(row, rng) for row in self.rows])

    def padded(self, r):
        return self.rows[r] + [0] * (self.n - self.n_valid)

    def entrance(self, r, p):
        return direct_transform(self.padded(r), self.max_logr, self.roots, self.W, self.inverse, until=p)

    def tree_of(self, mark):
        """the levels of the crafted output's sum tree, from the model"""
        r, p, j, u, off, a, kind = mark
        logr, ns, cols, n_terms, scale = self.pass_shape(p)
        state = self.entrance(r, p)
        return tree_levels([direct_coefficient(self.n, logr, ns, j, u, t, self.roots, self.W, scale) * state[j + t * cols] % R for t in range(n_terms)])

    def expected_dlogs(self, r):
        return direct_transform(self.padded(r), self.max_logr, self.roots, self.W, self.inverse)


# (n, max_logr, rows, later pass, n_valid): two full radix-16 passes / 8 . 8 . 4; 16 then 4 (a short last pass) / 8 . 8; the pruned tree
DIRECT_SHAPES = ((256, 4, 4, 1, None), (256, 3, 4, 2, None), (64, 4, 8, 1, None), (64, 3, 4, 1, None), (256, 4, 2, None, 128), (256, 3, 2, None, 128))


# ---------------------------------------------------------------------------------------------- through the public API: the whole network
NETWORK_STAGES = (2, 8, 32)          # an early, a middle and the last stage of a 64-point transform


class NetworkCase:
    """8 distinct 64-point rows; row d has collisions x == w y and x == -w y at four butterflies with j != 0 of stage NETWORK_STAGES[d % 3], placed in
    the state at that stage's entrance and pulled back through the earlier stages and the bit reversal.  (An INFINITE value at a stage's entrance
    is a collision of the stage before: those are the business of the one-stage cases.)"""

    def __init__(self, inverse, n=64, scale=STAGE_SCALE, rows=MAX_DISTINCT_ROWS, seed=0):
        self.n, self.inverse, self.W = n, inverse, 1 << scale
        expanded, reverse = tables(scale)
        self.roots = reverse if inverse else expanded
        rng = random.Random("network %d %d %d" % (n, inverse, seed))
        self.rows, self.marks = [], []
        for d in range(rows):
            m = NETWORK_STAGES[d % len(NETWORK_STAGES)]
            state = [rand_nz(rng) for _ in range(n)]
            slots = [(g, j, i0, i1) for g, j, i0, i1 in butterflies(n, m) if j != 0]
            for c, (g, j, i0, i1) in enumerate(rng.sample(slots, 4)):
                w = twiddle(self.roots, self.W, m, j)
                cls = STAGE_CLASSES_ANY_J[c % 2]
                state[i0] = (w if cls == "x==wy" else -w) * state[i1] % R
                self.marks.append((d, m, g, j, cls))
            self.rows.append(dit_pull_back(state, m, self.roots, self.W))

    def images(self):
        rng = random.Random("network images %d" % self.inverse)
        return np.stack([points(row, rng) for row in self.rows])

    def expected_dlogs(self, d):
        out = dit_network(self.rows[d], self.roots, self.W)
        return [v * inv(self.n) % R for v in out] if self.inverse else out
