"""Scenarios for the cooperative bucket kernels (pippenger.hpp k_pip_window / k_pip_window_seg): every exceptional branch of
the point addition at every step of the workgroup algorithm.  Shared by tests/test_pip_model.py (the table against the model,
no library), tests/test_pip_cases_hosttwin.py (the table and its references through the host twin's bucket stages) and
tests/test_pip_cases_gpu.py (the two kernels).

A scenario is ONE window of one workgroup: items (k, digit), the point of an item being k G (k = 0: the identity, given to
the library as the point (0, 0)).  tests/pip_model.py says which (site, branch) pairs a scenario meets; the oracle says what
its sum is.  The table is hand-built from a few shapes:
  single(b)            one non-empty bucket: identities on either side in the scan, the hop and the final additions, and equal
                       operands all the way down the tree (every suffix sum below b is the same point);
  same(b, off)         one point in buckets b and b + off: equal operands at scan:off, or -- across a wavefront border -- in
                       the hop;
  same_repr(b, off)    P1 and P2 in bucket b (a Jacobian sum with z != 1), P1 + P2 as one affine item in bucket b + off: the
                       same group element in two representations;
  opposite(b, off)     P and -P at those distances, and a third bucket elsewhere so that the window sum is not the identity;
  tree_two / final_three   two or three buckets whose logarithms are solved so that a partial sum of the tree, or of thread
                       0's last three additions, vanishes, coincides with or is opposite to its partner (formulas below);
  identity points with non-zero digits; buckets that cancel inside; a dense window (every bucket a different point);
  one bucket holding a whole tile: 4095, 4096 and 4097 items with one digit (4097: two tiles / segments; the uint16 index
  list of the first is full).
Logarithms are small integers (and their negatives) wherever the shape allows: k G is then cheap for the Python oracle."""
import functools
import random

import keyed_bv_cases as bv
import pip_model as pm

A, C2, P1, P2 = 1009, 2003, 3001, 4007               # logarithms of the points the small shapes are made of
BIG_SIZES = (4095, 4096, 4097)
SINGLE_BUCKETS = (1, 2, 63, 64, 65, 127, 128, 191, 192, 193, 254, 255)


class Scenario:
    def __init__(self, name, items, seq=False):
        self.name, self.items, self.seq = name, items, seq          # seq: the points are a prefix of the arithmetic sequence

    def __repr__(self):
        return "Scenario(%s)" % self.name


def _tree_two(r, wv, off, kind):
    """Buckets 64 wv + 63 (logarithm A) and 64 wv + off - 1 (logarithm c), nothing above wavefront wv.  Inside the wavefront
    the suffix sums are A above the lower bucket and A + c from it down.  At tree:off lane 0 holds the sum of the suffix sums
    of the lanes = 0 mod 2 off -- m = 32 / off of them, one of which (lane 0 itself) includes c: m A + c -- and receives that
    of the lanes = off mod 2 off, none of which does: m A.  c = -m A: p is the identity; c = -2 m A: the two are opposite."""
    m = 32 // off
    c = {"p identity": -m * A, "opposite": -2 * m * A}[kind] % r
    return [(A, 64 * wv + 63), (c, 64 * wv + off - 1)]


def _final_three(r, h_of):
    """Buckets 255 (A), 191 (C2) and 1 (h).  With s = A + C2 the four wavefronts' tree sums are W3 = 64 A, W2 = W1 = 64 s and
    W0 = 63 s + h, and thread 0 adds ((W0 + W1) + W2) + W3.  h_of(s) picks the relation:
      final:1  equal h = s           opposite h = -127 s          p identity h = -63 s
      final:2  equal h = -63 s       opposite h = -191 s          p identity h = -127 s
      final:3  equal h = 64 A - 191 s   opposite h = -64 A - 191 s   p identity h = -191 s"""
    s = A + C2
    return [(A, 255), (C2, 191), (h_of(s) % r, 1)]


def table(r):
    """The scenario table over the group order r (logarithms only; points come from Points below)."""
    t = []
    for b in SINGLE_BUCKETS:
        t.append(Scenario("single(%d)" % b, [(A, b)]))
    # a single bucket at in-wavefront lane off - 1: nothing reaches lane 0 from lane off at tree:off
    for wv, off in ((3, 32), (2, 16), (1, 8), (3, 4), (2, 2)):
        t.append(Scenario("single(%d)" % (64 * wv + off - 1), [(C2, 64 * wv + off - 1)]))
    pairs = [(64 * (i % 4) + 3, off) for i, off in enumerate(pm.SCAN_OFFS)] + [(63, 1), (127, 1), (191, 1), (40, 32), (100, 128)]
    for b, off in pairs:
        t.append(Scenario("same(%d, %d)" % (b, off), [(A, b), (A, b + off)]))
        t.append(Scenario("same_repr(%d, %d)" % (b, off), [(P1, b), (P2, b), (P1 + P2, b + off)]))
        third = 20 if b > 20 else 250                      # below both, so that it joins neither operand of the addition meant
        t.append(Scenario("opposite(%d, %d)" % (b, off), [(A, b), (r - A, b + off), (C2, third)]))
    # inside one bucket
    t.append(Scenario("bucket equal", [(A, 9), (A, 9)]))
    t.append(Scenario("bucket equal, three times", [(A, 201), (A, 201), (A, 201)]))
    t.append(Scenario("bucket equal, other representation", [(P1, 70), (P2, 70), (P1 + P2, 70)]))
    t.append(Scenario("bucket opposite", [(A, 9), (r - A, 9), (C2, 77)]))
    t.append(Scenario("bucket opposite, then on", [(A, 130), (r - A, 130), (C2, 130)]))
    t.append(Scenario("bucket generic", [(A, 9), (C2, 9), (P1, 9)]))
    t.append(Scenario("window cancels", [(A, 100), (r - A, 100)]))
    t.append(Scenario("buckets cancel", [(A, 100), (r - A, 100), (C2, 31), (r - C2, 31)]))
    # identity points with non-zero digits
    t.append(Scenario("identity points", [(0, 5), (A, 5), (0, 5), (0, 130), (C2, 200), (0, 255)]))
    t.append(Scenario("identity points alone", [(0, 7), (0, 255), (0, 64)]))
    t.append(Scenario("empty window", [(A, 0), (C2, 0)]))
    # the tree
    for i, off in enumerate(pm.TREE_OFFS):
        for kind in ("p identity", "opposite"):
            wv = 1 + i % 3
            t.append(Scenario("tree_two(wave %d, %d, %s)" % (wv, off, kind), _tree_two(r, wv, off, kind)))
    # thread 0's last three additions
    for name, h_of in (("h = s", lambda s: s), ("h = -63 s", lambda s: -63 * s), ("h = -127 s", lambda s: -127 * s),
                       ("h = -191 s", lambda s: -191 * s), ("h = 64 A - 191 s", lambda s: 64 * A - 191 * s),
                       ("h = -64 A - 191 s", lambda s: -64 * A - 191 * s)):
        t.append(Scenario("final_three(%s)" % name, _final_three(r, h_of)))
    t.append(Scenario("final: wavefronts 1 and 2 sum to the identity", [(A, 255), (r - A, 191), (C2, 1)]))
    return t


def seq_logs(r, n=BIG_SIZES[-1], seed=41):
    """The logarithms of the arithmetic sequence keyed_bv_cases.arithmetic_points draws with random.Random(seed)."""
    rng = random.Random(seed)
    s0, d = rng.randrange(1, r), rng.randrange(1, r)
    return [(s0 + i * d) % r for i in range(n)]


def seq_table(r):
    """The scenarios whose points are a prefix of the arithmetic sequence: every bucket a different point (digit i + 1 for
    item i; and 300 items with drawn digits), and the whole-tile buckets."""
    logs = seq_logs(r)
    rng = random.Random(43)
    t = [Scenario("dense", [(logs[i], i + 1) for i in range(255)], seq=True),
         Scenario("dense, drawn digits", [(logs[i], rng.randrange(256)) for i in range(300)], seq=True)]
    for n, d in zip(BIG_SIZES, (200, 1, 255)):
        t.append(Scenario("one bucket, %d items" % n, [(logs[i], d) for i in range(n)], seq=True))
    return t


def is_big(s):
    return len(s.items) >= BIG_SIZES[0]


# A (site, branch) pair that no input can reach, each with its one-line argument.  No "generic" entry and no site as a whole
# may stand here (tests/test_pip_model.py checks both).  Empty: every addition of the walk has two operands that the buckets'
# contents determine freely, so each of the five relations between them has a scenario in the table.
UNREACHABLE = {}


class Points:
    """k G for the logarithms of the tables, by the oracle: small |k| by one short multiplication, the arithmetic sequence by
    additions (keyed_bv_cases.arithmetic_points)."""

    def __init__(self, c):
        self.c = c
        self.cache = {0: None}
        self.seq, logs = bv.arithmetic_points(c, BIG_SIZES[-1], random.Random(41))
        assert logs == seq_logs(c.r)

    def get(self, k):
        c = self.c
        k %= c.r
        if k not in self.cache:
            small = min(k, c.r - k)
            p = c.g1_mul(c.g1, small)
            self.cache[small], self.cache[c.r - small] = p, c.g1_neg(p)
        return self.cache[k]

    def of(self, s):
        return self.seq[:len(s.items)] if s.seq else [self.get(k) for k, _ in s.items]

    def window_sum(self, s):
        """The reference: one multiplication of the generator by sum digit_i k_i."""
        return self.get(pm.plain_sum(s.items, self.c.r))

    def term_by_term(self, s):
        """The same sum as the definition reads, every product digit * P_i by the oracle (small scenarios)."""
        c, acc = self.c, None
        for p, (_, d) in zip(self.of(s), s.items):
            if d and p is not None:
                acc = c.g1_add(acc, c.g1_mul(p, d))
        return acc


@functools.lru_cache(maxsize=None)
def scene(curve):
    """(curve object, Points, small scenarios, sequence scenarios): built once per curve."""
    from oracle import bbs
    c = bbs.SUITES[curve].curve
    return c, Points(c), table(c.r), seq_table(c.r)


def packed_groups(pts, scenarios, per_group=16):
    """bbs_selftest_segmented_sums input: `per_group` scenarios per group, scenario j of a group in window j -- its items carry
    their digit in that window and 0 in every other.  -> (points, digits[16][n], groups, slots) with slots[j] = (group, window)
    of scenario j."""
    points, cols, groups, slots = [], [], [], []
    for g0 in range(0, len(scenarios), per_group):
        first = len(points)
        for w, s in enumerate(scenarios[g0:g0 + per_group]):
            for p, (_, d) in zip(pts.of(s), s.items):
                points.append(p)
                cols.append((w, d))
            slots.append((len(groups), w))
        groups.append((first, len(points) - first))
    digits = [[d if w == cw else 0 for cw, d in cols] for w in range(16)]
    return points, digits, groups, slots


def msm_input(pts, scenarios):
    """bbs_g1_msm_pippenger input: up to 30 scenarios, scenario j as byte j of the scalars (bytes 30 and 31 stay 0, so every
    scalar is below the group order).  -> (points, scalars, logarithm of the expected sum = sum_j 256^j S_j)."""
    assert len(scenarios) <= 30
    points, scalars, want = [], [], 0
    for j, s in enumerate(scenarios):
        for p, (_, d) in zip(pts.of(s), s.items):
            points.append(p)
            scalars.append(d << (8 * j))
        want += pm.plain_sum(s.items, pts.c.r) << (8 * j)
    return points, scalars, want % pts.c.r


# ---- the two legs, shared by the host-twin and the GPU test ------------------------------------------------------------------
def references(curve):
    """{scenario name: expected window sum}, computed once per curve: one multiplication of the generator per scenario, and
    for the scenarios of at most six items the sum term by term as well."""
    return _references(curve)


@functools.lru_cache(maxsize=None)
def _references(curve):
    c, pts, small, seq = scene(curve)
    want = {}
    for s in small + seq:
        want[s.name] = pts.window_sum(s)
        assert want[s.name] == pts.get(pm.window_sum(s.items, c.r)[0]), s
        if len(s.items) <= 6:
            assert pts.term_by_term(s) == want[s.name], s
    return want


def check_segmented_sums(eng, curve):
    """Every scenario as one window of a group of bbs_selftest_segmented_sums (product: k_pip_window_seg): 16 small scenarios
    per group; the two dense ones share a group; a whole-tile bucket is a group of its own, in window 0."""
    c, pts, small, seq = scene(curve)
    want = references(curve)
    order = small + [s for s in seq if not is_big(s)]
    points, digits, groups, slots = packed_groups(pts, order)
    got = eng.segmented_sums(points, digits, groups)
    bad = [s.name for s, (g, w) in zip(order, slots) if got[g][w] != want[s.name]]
    assert not bad, (curve, bad)
    # windows no scenario stands in sum to the identity
    used = set(slots)
    assert all(got[g][w] is None for g in range(len(groups)) for w in range(16) if (g, w) not in used)
    for s in (s for s in seq if is_big(s)):
        points, digits, groups, _ = packed_groups(pts, [s])
        got = eng.segmented_sums(points, digits, groups)
        assert got[0][0] == want[s.name], (curve, s)
        assert all(p is None for p in got[0][1:]), (curve, s)


def check_msm(eng, curve):
    """The same digits as bytes 0 .. 29 of the scalars of bbs_g1_msm_pippenger (product: k_pip_window, then PipTileSums with
    the 2^(8 w) shifts): 30 scenarios per call, a whole-tile bucket in a call of its own."""
    c, pts, small, seq = scene(curve)
    order = small + [s for s in seq if not is_big(s)]
    calls = [order[k:k + 30] for k in range(0, len(order), 30)] + [[s] for s in seq if is_big(s)]
    for call in calls:
        points, scalars, want = msm_input(pts, call)
        got, st = eng.g1_msm_pippenger(points, scalars)
        assert list(st) == [1] * len(points), (curve, call[0])
        assert got == pts.get(want), (curve, [s.name for s in call])
