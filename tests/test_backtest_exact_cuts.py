"""The two exact cuts of the backtest lane loop, emulated in f32 numpy.

(a) BtAccum::mark (ops/hip/bt_common.hpp) skips the drawdown divide when
    x = max_eq - equity satisfies x <= fl(max_eq * fl(max_dd * C)), C =
    1 - 2^-23. The emulation must never skip a divide that would have
    raised max_dd — and with C = 1 it must, which shows that the margin is
    needed and that the triples sit on the boundary.
(b) bt_vote_flip (ops/hip/bt_vote.hpp) finds, per candle, the parameter at
    which a stochastic / Williams vote flips, so that a lane compares its
    parameter with it instead of multiplying. A numpy port of the search
    is held to equality with the multiply-and-compare form, vote for vote.
"""

import numpy as np
import pytest

f32 = np.float32
C_GUARD = f32(1.0) - f32(2.0 ** -23)
BT_EPS = f32(1e-9)


# ------------------------------------------------------------- (a) guard
def _ulp_shift(a, k):
    """a moved by k units in the last place (positive finite a)."""
    return (a.view(np.int32) + k.astype(np.int32)).view(np.float32)


def _guard_triples(n, seed):
    """(max_eq, max_dd, x) with x within +-6 ulp of fl(max_eq * max_dd),
    max_eq log-uniform over 1e-3 .. 1e4, max_dd from 2^-24 (its smallest
    non-zero value) to 1."""
    rng = np.random.default_rng(seed)
    m = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n)).astype(f32)
    d = np.exp(rng.uniform(np.log(2.0 ** -24), 0.0, n)).astype(f32)
    d = _ulp_shift(d, rng.integers(-2, 3, n))
    x = _ulp_shift((m * d).astype(f32), rng.integers(-6, 7, n))
    return m, d, x


def _wrong_skips(m, d, x, c):
    with np.errstate(all="ignore"):
        thr = (m * (d * f32(c)).astype(f32)).astype(f32)
        skip = x <= thr
        raised = (x / m).astype(f32) > d       # the divide would raise max_dd
    return skip & raised, skip


def test_guard_never_skips_a_raising_divide():
    m, d, x = _guard_triples(4_000_000, seed=1)
    wrong, skip = _wrong_skips(m, d, x, C_GUARD)
    assert not wrong.any()
    # the triples straddle the boundary: both outcomes are common
    assert 0.2 < skip.mean() < 0.8
    # C = 1 - 2^-22 is safe as well
    assert not _wrong_skips(m, d, x, f32(1.0) - f32(2.0 ** -22))[0].any()


def test_guard_margin_is_necessary():
    m, d, x = _guard_triples(4_000_000, seed=1)
    wrong, _ = _wrong_skips(m, d, x, f32(1.0))
    assert wrong.sum() > 100


def test_guard_zeros_new_highs_and_ties():
    rng = np.random.default_rng(2)
    n = 200_000
    m = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n)).astype(f32)
    zero = np.zeros(n, f32)
    d = rng.uniform(0.0, 0.9, n).astype(f32)
    # max_dd == 0: the threshold is 0, only x == 0 skips
    below = (m - np.nextafter(m, f32(0))).astype(f32)    # smallest x > 0
    wrong, skip = _wrong_skips(m, zero, below, C_GUARD)
    assert not wrong.any() and not skip.any()
    wrong, skip = _wrong_skips(m, zero, zero, C_GUARD)
    assert not wrong.any() and skip.all()
    # a new high: x == 0 against any max_dd
    wrong, skip = _wrong_skips(m, d, zero, C_GUARD)
    assert not wrong.any() and skip[d > 0].all()
    # ties: max_dd is exactly the quotient of the triple
    x = (m * d).astype(f32)
    tie = (x / m).astype(f32)
    wrong, _ = _wrong_skips(m, tie, x, C_GUARD)
    assert not wrong.any()
    # the guard switched off (dd_c == 0): only x == 0 skips
    wrong, skip = _wrong_skips(m, d, x, f32(0.0))
    assert not wrong.any() and not skip[x > 0].any()
    # NaN falls through to the divide
    nan = np.full(n, np.nan, f32)
    assert not _wrong_skips(m, d, nan, C_GUARD)[1].any()
    assert not _wrong_skips(nan, d, x, C_GUARD)[1].any()
    assert not _wrong_skips(m, nan, x, C_GUARD)[1].any()


@pytest.mark.parametrize("eq0", [1e-3, 1.0, 1e4])
def test_guarded_mark_equals_always_divide(eq0):
    """mark() over random equity walks with long slides, both forms: the
    running max_dd is the same f32 after every candle."""
    rng = np.random.default_rng(3)
    lanes, T = 4096, 600
    equity = np.full(lanes, eq0, f32)
    max_eq = equity.copy()
    dd_ref = np.zeros(lanes, f32)
    dd_new = np.zeros(lanes, f32)
    drift = rng.choice([-0.004, 0.0, 0.003], lanes).astype(f32)
    skipped = 0
    for _ in range(T):
        step = (drift + 0.003 * rng.standard_normal(lanes)).astype(f32)
        step[rng.random(lanes) < 0.2] = 0.0            # equity stands still
        equity = (equity * (f32(1) + step)).astype(f32)
        max_eq = np.maximum(max_eq, equity)
        x = (max_eq - equity).astype(f32)
        dd_ref = np.maximum(dd_ref, (x / max_eq).astype(f32))
        skip = x <= (max_eq * (dd_new * C_GUARD).astype(f32)).astype(f32)
        dd_new = np.where(skip, dd_new,
                          np.maximum(dd_new, (x / max_eq).astype(f32)))
        skipped += skip.sum()
        assert np.array_equal(dd_new, dd_ref)
    assert skipped > 0.5 * lanes * T                   # the guard does work


# -------------------------------------------------------- (b) thresholds
KEY_INF = 0x7f800000


def key_to_f32(k):
    """bt_key: ordered-integer image -> float (k as int64)."""
    k = np.asarray(k, np.int64)
    bits = np.where(k >= 0, k, 0x80000000 - k) & 0xffffffff
    return bits.astype(np.uint32).view(np.float32)


def f32_to_key(f):
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u < 0x80000000, u, 0x80000000 - u)


def _q(k, num, s, sell):
    with np.errstate(all="ignore"):
        f = (key_to_f32(k) * s).astype(f32)
    return ~(num > f) if sell else (num < f)


def vote_flip(num, s, est, sell):
    """Port of bt_vote_flip: key of the first float p with Q(p) true."""
    klow, khigh = -KEY_INF, KEY_INF
    k0 = np.clip(f32_to_key(est), klow + 1, khigh - 1)
    down = _q(k0, num, s, sell)
    lo = np.where(down, klow, k0)
    hi = np.where(down, k0, khigh)
    step = np.ones_like(k0)
    active = np.ones(k0.shape, bool)
    while True:
        active &= step < np.where(down, hi - klow, khigh - lo)
        if not active.any():
            break
        c = np.where(down, hi - step, lo + step)
        qc = _q(c, num, s, sell)
        lo = np.where(active & ~qc, c, lo)
        hi = np.where(active & qc, c, hi)
        active &= qc == down
        step = np.where(active, step * 2, step)
    while True:
        wide = hi - lo > 1
        if not wide.any():
            break
        mid = lo + (hi - lo) // 2
        qm = _q(mid, num, s, sell)
        hi = np.where(wide & qm, mid, hi)
        lo = np.where(wide & ~qm, mid, lo)
    return hi


def vote_thresholds(num, s):
    """Port of bt_vote_thresholds: (theta_buy, theta_sell)."""
    with np.errstate(all="ignore"):
        est = (num * (f32(1) / s).astype(f32)).astype(f32)
    return (key_to_f32(vote_flip(num, s, est, False)),
            key_to_f32(vote_flip(num, s, est, True) - 1))


def _candles(seed, n):
    """(close, lmin, hmax) of n candles: random ranges at price levels
    1e-2 .. 1e4, then the edge cases — close == lmin, close == hmax, a
    flat range (srange = eps)."""
    rng = np.random.default_rng(seed)
    level = np.exp(rng.uniform(np.log(1e-2), np.log(1e4), n)).astype(f32)
    lmin = (level * (1 - rng.uniform(0, 0.02, n))).astype(f32)
    hmax = (level * (1 + rng.uniform(0, 0.02, n))).astype(f32)
    cl = (lmin + (hmax - lmin) * rng.uniform(0, 1, n)).astype(f32)
    cl = np.clip(cl, lmin, hmax)
    kind = rng.integers(0, 8, n)
    cl = np.where(kind == 0, lmin, cl)
    cl = np.where(kind == 1, hmax, cl)
    flat = kind == 2
    lmin = np.where(flat, cl, lmin)
    hmax = np.where(flat, cl, hmax)
    return cl, lmin, hmax


def _numerators(cl, lmin, hmax):
    st_num = (f32(100) * (cl - lmin)).astype(f32)
    wl_num = (f32(-100) * (hmax - cl)).astype(f32)
    srange = np.maximum((hmax - lmin).astype(f32), BT_EPS)
    return st_num, wl_num, srange


def _lane_params(theta, rng, per=24):
    """Lane parameters for each candle: +-4 ulp around theta (in the
    ordered-integer image, so across zero and into the subnormals), and
    uniform over [-200, 200]."""
    k = f32_to_key(np.where(np.isfinite(theta), theta, f32(0)))
    near = k[:, None] + np.arange(-4, 5)[None, :]
    near = np.clip(near, -KEY_INF + 1, KEY_INF - 1)
    wide = rng.uniform(-200, 200, (len(theta), per)).astype(f32)
    return np.concatenate([key_to_f32(near), wide], axis=1)


def _assert_votes_equal(num, s, rng):
    th_b, th_s = vote_thresholds(num, s)
    for theta in (th_b, th_s):
        p = _lane_params(theta, rng)
        with np.errstate(all="ignore"):
            prod = (p * s[:, None]).astype(f32)
        assert np.array_equal(num[:, None] < prod, p >= th_b[:, None])
        assert np.array_equal(num[:, None] > prod, p <= th_s[:, None])
    return th_b, th_s


def test_thresholds_equal_multiply_and_compare():
    """All four votes of a candle: stochastic on st_num, Williams on
    wl_num, a lane's Williams parameter being its own stoch - 100."""
    rng = np.random.default_rng(5)
    cl, lmin, hmax = _candles(4, 20_000)
    st_num, wl_num, s = _numerators(cl, lmin, hmax)
    assert (st_num == 0).any() and (wl_num == 0).any() and (s == BT_EPS).any()
    assert np.signbit(wl_num[wl_num == 0]).any()        # -0 numerators
    _assert_votes_equal(st_num, s, rng)
    th_b, th_s = _assert_votes_equal(wl_num, s, rng)
    # the lane's form: will = stoch - 100, both Williams votes
    stoch = rng.uniform(0, 100, (len(s), 16)).astype(f32)
    will = (stoch - f32(100)).astype(f32)
    prod = (will * s[:, None]).astype(f32)
    assert np.array_equal(wl_num[:, None] < prod, will >= th_b[:, None])
    assert np.array_equal(wl_num[:, None] > prod, will <= th_s[:, None])


def test_thresholds_at_the_edges_of_f32():
    """+-0 numerators, the flat range, products that underflow or
    overflow, every finite numerator size: the gallop-and-bisect
    fall-back. theta is checked directly too: Q holds at it and fails
    one float before."""
    rng = np.random.default_rng(6)
    tiny = f32(1e-45)
    big = np.finfo(f32).max
    nums = np.array([0.0, -0.0, tiny, -tiny, 1e-40, -1e-40, 1e-30, -3e-22,
                     1.0, -1.0, 7e3, -7e3, 1e30, -1e30, big, -big], f32)
    ss = np.array([BT_EPS, 1e-40, tiny, 1e-6, 0.37, 1.0, 250.0, 1e20, big],
                  f32)
    num = np.repeat(nums, len(ss))
    s = np.tile(ss, len(nums))
    th_b, th_s = _assert_votes_equal(num, s, rng)
    for sell, key in ((False, f32_to_key(th_b)), (True, f32_to_key(th_s) + 1)):
        inf = np.isinf(th_b if not sell else th_s)
        fin = ~inf
        assert _q(key[fin], num[fin], s[fin], sell).all()
        prev = key[fin] - 1
        inside = prev > -KEY_INF
        assert not _q(prev[inside], num[fin][inside], s[fin][inside],
                      sell).any()
    # +inf / -inf exactly where no finite parameter takes the vote
    with np.errstate(all="ignore"):
        top = (big * s).astype(f32)
        bottom = (-big * s).astype(f32)
    assert np.array_equal(np.isposinf(th_b), ~(num < top))
    assert np.array_equal(np.isneginf(th_s), ~(num > bottom))
