"""The workgroup algorithm of the cooperative bucket kernels (bbs_sign_amd/csrc/pippenger.hpp k_pip_window and
k_pip_window_seg, steps 2 - 5) walked on discrete logarithms.

A test that knows every point of a window as a multiple k_i G of one base can say on plain integers mod r which addition of
the kernel takes which branch of g1j_add / g1j_add_aff: the identity on either side, equal operands (the doubling), opposite
operands (the identity comes out), or the generic formula.  That is all this module does.  It serves COVERAGE only: it says
which branch a scenario enters; right or wrong is always decided by the oracle.  (Two equal group elements with different
Jacobian coordinates take the same branch; that they do is what the scenarios with a two-item bucket beside a one-item
bucket are for -- the model cannot see coordinates and does not try.)

The walk, as the kernels do it for one (point set, window, tile of at most 4096 items), thread b owning bucket b:
  bucket     thread b adds its members in item order with g1j_add_aff(acc, P_i), from the identity;
  scan:off   off = 1, 2, .. 32: thread b takes the value of lane + off of ITS wavefront (all at once) and, if lane + off < 64,
             acc = g1j_add(acc, that) -- the suffix sums inside a wavefront;
  hop        the four wavefronts' lane 0 values V_k go through LDS; thread b of wavefront wv forms above = ((O + V_3) + V_2) ..
             down to V_(wv + 1) and then acc = g1j_add(acc, above) -- every addition of both kinds is site "hop";
  (thread 0's value, the suffix sum of bucket 0, is replaced by the identity)
  tree:off   off = 32, 16, .. 1: lanes below off add the value of lane + off of their wavefront;
  final:k    k = 1, 2, 3: thread 0 adds wavefront k's lane 0 value.
A branch is named as g1j_add(p, q) decides it, in its order: "q identity" (q is the identity, whatever p), "p identity",
"equal", "opposite", "generic".  The identity is the logarithm 0.

Pure Python, no library."""

TILE = 4096
SCAN_OFFS = (1, 2, 4, 8, 16, 32)
TREE_OFFS = (32, 16, 8, 4, 2, 1)
SITES = ("bucket",) + tuple("scan:%d" % o for o in SCAN_OFFS) + ("hop",) + tuple("tree:%d" % o for o in TREE_OFFS) + \
    tuple("final:%d" % k for k in (1, 2, 3))
BRANCHES = ("q identity", "p identity", "equal", "opposite", "generic")
ALL_PAIRS = frozenset((s, b) for s in SITES for b in BRANCHES)


def _add(p, q, r, site, met):
    """g1j_add(p, q) / g1j_add_aff(p, q) on logarithms: the sum, with the branch recorded."""
    if q == 0:
        met.add((site, "q identity"))
        return p
    if p == 0:
        met.add((site, "p identity"))
        return q
    if p == q:
        met.add((site, "equal"))
    elif (p + q) % r == 0:
        met.add((site, "opposite"))
    else:
        met.add((site, "generic"))
    return (p + q) % r


def tile_sum(items, r, met):
    """One workgroup: items = [(k, digit)] of one tile in item order -> the logarithm of sum digit_i * k_i G."""
    assert len(items) <= TILE
    acc = [0] * 256
    for k, d in items:                                   # membership (digit 0: no bucket) and the bucket sums, item order
        assert 0 <= d < 256 and 0 <= k < r
        if d:
            acc[d] = _add(acc[d], k, r, "bucket", met)
    for off in SCAN_OFFS:                                # Hillis-Steele suffix scan inside each wavefront
        old = list(acc)
        for b in range(256):
            if (b & 63) + off < 64:
                acc[b] = _add(old[b], old[b + off], r, "scan:%d" % off, met)
    v = [acc[64 * k] for k in range(4)]                  # s_pt: what lane 0 of every wavefront holds
    for b in range(256):
        wv, above = b >> 6, 0
        for k in range(3, wv, -1):
            above = _add(above, v[k], r, "hop", met)
        acc[b] = _add(acc[b], above, r, "hop", met)
    acc[0] = 0                                           # bucket 0's suffix sum is not a term
    for off in TREE_OFFS:
        old = list(acc)
        for b in range(256):
            if (b & 63) < off:
                acc[b] = _add(old[b], old[b + off], r, "tree:%d" % off, met)
    total = acc[0]
    for k in (1, 2, 3):
        total = _add(total, acc[64 * k], r, "final:%d" % k, met)
    return total


def window_sum(items, r):
    """A scenario (items with logarithm and digit, any number) -> (logarithm of the window sum, the (site, branch) pairs met).
    More than one tile: the kernels run one workgroup per 4096 items and a lane functor adds their sums (PipTileSums /
    PipGroupSums, which are not sites of this model)."""
    met = set()
    total = 0
    for first in range(0, max(len(items), 1), TILE):
        total = (total + tile_sum(items[first:first + TILE], r, met)) % r
    return total, met


def plain_sum(items, r):
    return sum(d * k for k, d in items) % r
