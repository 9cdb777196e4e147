"""The 16 combined checks of batch verification on the GPU (tests/bv_verdict_cases.py; every expectation is proved on the host
twin by tests/test_bv_verdicts_hosttwin.py first).  Here the combination is the product's: RlcPrep / PvChallengeBv, the
cooperative bucket kernel k_pip_window with two point sets -- its out_aff branch for one tile, PipTileSums for two -- and the
sixteen split pairing checks.  An all-valid job must show sixteen verdicts at 1: a combination that is wrong in the failing
direction would leave every status right (the per-item kernel decides) and only the benchmark's rate would move.

Sizes: below, at and above a 64-digit chunk and the 256 buckets; 4097 = two tiles, once per curve.  L = 4, R = 2."""
import functools

import pytest

import bv_verdict_cases as vc

pytestmark = pytest.mark.gpu

L, R = 4, 2
BIG = 4097
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
FORMS = [pytest.param(False, id="throughput"), pytest.param(True, id="latency", marks=pytest.mark.job_form(True))]
# 17 forged items among 40: first and last item included, runs and gaps of several lengths
FORGED17 = [0, 1, 2, 5, 7, 8, 12, 15, 16, 19, 23, 24, 29, 31, 32, 36, 39]


@functools.lru_cache(maxsize=None)
def _scene(curve):
    """(issuer, 4097 valid items): made once per curve, never changed; the smaller jobs are its prefixes."""
    return vc.make_batch(curve, BIG, L, R, None, seed=29)


@pytest.mark.parametrize("latency", FORMS)
@pytest.mark.parametrize("curve", vc.CURVES)
def test_all_valid_one_tile(curve, latency):
    iss, base = _scene(curve)
    on, off = vc.engines(iss)
    for n in SIZES:
        batch = vc.take(base, range(n))
        for op in vc.OPS:
            vc.check_all_valid(iss, batch, on, off, op, latency, sample=[n - 1] if n in (1, 65, 257) else ())


@pytest.mark.parametrize("curve", vc.CURVES)
def test_all_valid_two_tiles(curve):
    iss, base = _scene(curve)
    on, off = vc.engines(iss)
    for op in vc.OPS:
        vc.check_all_valid(iss, base, on, off, op, sample=[0, 4095, 4096])


@pytest.mark.parametrize("latency", FORMS)
@pytest.mark.parametrize("curve", vc.CURVES)
def test_failures_before_the_pairing(curve, latency):
    iss, base = _scene(curve)
    on, off = vc.engines(iss)
    batch = vc.take(base, range(70))
    for i in (0, 64, 69):
        vc.check_wrong_challenge_scalar(iss, batch, on, off, latency, i)
        vc.check_replaced_abar(iss, batch, on, off, latency, i)
    for op in vc.OPS:
        vc.check_nothing_reaches_the_pairing(iss, batch, on, off, op, latency)


@pytest.mark.parametrize("latency", FORMS)
@pytest.mark.parametrize("curve", vc.CURVES)
def test_forged_items(curve, latency):
    iss, base = _scene(curve)
    on, off = vc.engines(iss)
    valid = vc.take(base, range(130))
    for bad in (0, 129, 63, 64):
        batch = valid.copy().make_bad([bad])
        for op in vc.OPS:
            vc.check_rejected(iss, batch, on, off, op, {bad}, latency, sample=[bad])


@pytest.mark.parametrize("keyed", [False, True], ids=["single_key", "keyed"])
@pytest.mark.parametrize("curve", vc.CURVES)
def test_repeated_item(curve, keyed):
    """n copies of one valid item: every non-empty bucket holds the same point n_b times, so the bucket sums are multiples of
    one point and the scan and the tree meet equal operands (the doubling branch of the addition) wherever two of them agree."""
    iss, base = _scene(curve)
    on, off = vc.keyed_engines(iss) if keyed else vc.engines(iss)
    for n in (65, 257):
        for op in vc.OPS:
            vc.check_all_valid(iss, vc.repeated(base, n, src=7), on, off, op, keyed=keyed)


@pytest.mark.parametrize("keyed", [False, True], ids=["single_key", "keyed"])
@pytest.mark.parametrize("curve", vc.CURVES)
def test_cancelling_pairs(curve, keyed):
    """One item duplicated with A + T and A - T, in one 64-item chunk and in different chunks, and three copies of each
    sign: the errors cancel under equal coefficients, so a passing check here is a coefficient that does not depend on the
    item.  Both copies rejected, every other item accepted."""
    iss, base = _scene(curve)
    on, off = vc.keyed_engines(iss) if keyed else vc.engines(iss)
    valid = vc.take(base, range(130))
    for plus, minus in (([3], [40]), ([3], [100]), ([129], [0]), ([1, 70, 129], [2, 64, 128])):
        batch = vc.cancelling(valid, plus, minus, src=plus[0])
        for op in vc.OPS:
            vc.check_rejected(iss, batch, on, off, op, set(plus + minus), keyed=keyed, sample=[plus[0], minus[0]])


@pytest.mark.parametrize("keyed", [False, True], ids=["single_key", "keyed"])
@pytest.mark.parametrize("curve", vc.CURVES)
def test_cancelling_pair_across_tiles(curve, keyed):
    iss, base = _scene(curve)
    on, off = vc.keyed_engines(iss) if keyed else vc.engines(iss)
    batch = vc.cancelling(base, [10], [4096], src=10)
    for op in vc.OPS:
        vc.check_rejected(iss, batch, on, off, op, {10, 4096}, keyed=keyed, sample=[10, 4096])


@pytest.mark.parametrize("w", range(16))
@pytest.mark.parametrize("curve", vc.CURVES)
def test_exactly_one_window_fails(curve, w):
    """17 forged items among 40 whose errors cancel in every window but w (bv_verdict_cases.one_window_job): verdict w alone
    is 0, every forged item is rejected and every valid one accepted.  A decision that skipped flag w, a digit row read at
    another offset, or sums of window w that went to another slot would all show here."""
    iss, base = _scene(curve)
    on, off = vc.engines(iss)
    vc.check_one_window(iss, vc.take(base, range(40)), FORGED17, w, on, off)


@functools.lru_cache(maxsize=None)
def _two_key_scene(curve):
    """Items 0 .. 69 alternate between two keys: two groups of 35, in runs that the bv order sorts apart."""
    return vc.make_two_key_batch(curve, [i % 2 for i in range(70)], L, R, None, seed=31)


@pytest.mark.parametrize("w", range(16))
@pytest.mark.parametrize("curve", vc.CURVES)
def test_exactly_one_window_fails_keyed(curve, w):
    """The keyed group form: 17 of group w % 2's 35 items are forged so that its window w alone fails -- entry g * 16 + w of
    the 32 verdicts, and nothing of the other group."""
    iss, base = _two_key_scene(curve)
    g = w % 2
    mine = [i for i in range(70) if i % 2 == g]
    vc.check_one_window_keyed(iss, base, mine[:3] + mine[-14:], w, group=g)
