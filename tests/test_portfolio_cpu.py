"""The portfolio position machine's CPU twin
(backtesting/engine_portfolio_cpu.py) against its contract
(backtesting/portfolio.py): the single-symbol anchor, the zero-padded tree
sum, the ordering rules on hand-built flags, and account invariants on
random ones. Every comparison is exact: floats as bit patterns."""

import numpy as np
import pytest

import portfolio_cases as pc
from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
from ai_crypto_trader_amd.backtesting.engine_portfolio_cpu import (
    run_portfolio_backtest_cpu, run_portfolio_from_flags_cpu,
)
from ai_crypto_trader_amd.backtesting.portfolio import tree_sum64
from ai_crypto_trader_amd.backtesting.strategy import (
    DEFAULT_PARAMS, FEE, random_population,
)

f32 = np.float32
bits = pc.bits


def _market(T, nsym, seed):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(T, nsym, seed=seed))


# ---------------------------------------------------------------------
# single-symbol anchor
# ---------------------------------------------------------------------
def test_single_symbol_is_the_vote_backtest():
    candles = _market(1500, 1, seed=3)
    pop = random_population(16, seed=5)
    ref = run_backtest_cpu(candles, pop)[:, 0, :]
    assert ref[:, 1].sum() > 0
    res = run_portfolio_backtest_cpu(candles, pop, max_positions=1)
    assert (bits(res.metrics) == bits(ref)).all()
    assert (res.refused == 0).all()
    assert (bits(res.per_symbol[:, 0, :]) == bits(ref[:, 1:5])).all()
    assert res.equity is None


# ---------------------------------------------------------------------
# the tree sum
# ---------------------------------------------------------------------
def test_tree_sum_is_the_xor_butterfly():
    """Every lane of a 6-step xor reduction over 64 lanes, on values whose
    sum depends on the order (a left-to-right sum differs)."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 7, 33, 64):
        x = (rng.random(n) * 10.0 ** rng.integers(-3, 4, n)).astype(f32)
        v = np.zeros(64, f32)
        v[:n] = x
        for k in range(6):
            v = v + v[np.arange(64) ^ (1 << k)]
        assert (bits(v) == bits(v[:1])).all()
        assert bits(tree_sum64(x)) == bits(v[0])
    x = (rng.random(64) * 10.0 ** rng.integers(-3, 4, 64)).astype(f32)
    serial = f32(0.0)
    for a in x:
        serial = f32(serial + a)
    assert bits(tree_sum64(x)) != bits(serial)


@pytest.mark.parametrize("base, total", [(1, 2), (3, 64)])
def test_idle_symbols_change_nothing(base, total):
    """Symbols at a constant price whose flags are never set, appended to a
    basket: the same metrics, bit for bit, at the same max_positions. (The
    planes are given, not voted: the vote machine does vote on a constant
    price — RSI, Bollinger and stochastic all read it as oversold.)"""
    P, T = 12, 600
    candles, pop, ef, xf = pc.make_case(base, P, T, seed=21)
    kw = dict(max_positions=base, initial_equity=100.0, equity_stride=1)
    small = run_portfolio_from_flags_cpu(candles, pop, ef, xf, **kw)
    assert small.metrics[:, 1].sum() > 0
    idle = np.ones((total - base, T, 4), f32)
    idle[:, :, 0:3] = f32(3.25)
    pad = np.zeros((P, total - base, T), bool)
    big = run_portfolio_from_flags_cpu(
        np.concatenate([candles, idle]), pop,
        np.concatenate([ef, pad], axis=1),
        np.concatenate([xf, pad], axis=1), **kw)
    assert (bits(big.metrics) == bits(small.metrics)).all()
    assert (bits(big.equity) == bits(small.equity)).all()
    assert (big.refused == small.refused).all()
    assert (bits(big.per_symbol[:, :base]) == bits(small.per_symbol)).all()
    assert (big.per_symbol[:, base:] == 0).all()


# ---------------------------------------------------------------------
# directed ordering: 3 symbols at a flat price of 1, one strategy with
# stop 0.875 and take-profit 1.25 (exact in f32), no trailing stop
# ---------------------------------------------------------------------
T_DIR = 24


def _directed(size_pct, entries, exits, max_positions, lows=()):
    """entries / exits: (symbol, candle) pairs; lows: (symbol, candle, low)."""
    candles = np.ones((3, T_DIR, 4), f32)
    for s, t, lo in lows:
        candles[s, t, 2] = lo
    pop = DEFAULT_PARAMS.copy()[None]
    pop[0, 12:17] = (size_pct, 0.125, 0.25, 0.0, 0.0)
    ef = np.zeros((1, 3, T_DIR), bool)
    xf = np.zeros((1, 3, T_DIR), bool)
    for s, t in entries:
        ef[0, s, t] = True
    for s, t in exits:
        xf[0, s, t] = True
    return run_portfolio_from_flags_cpu(
        candles, pop, ef, xf, max_positions=max_positions, trace=True)


def test_lower_index_enters_first_and_the_other_is_refused_for_slots():
    res, tr = _directed(0.5, [(0, 5), (1, 5)], [(0, 10), (1, 10)], 1)
    assert res.refused.tolist() == [[1, 0]]
    assert tr["n_open"][0, 4:11].tolist() == [0, 1, 1, 1, 1, 1, 0]
    assert res.per_symbol[0, :, 0].tolist() == [1.0, 0.0, 0.0]
    assert res.metrics[0, 1] == 1.0


def test_an_exit_funds_an_entry_on_the_same_candle():
    """All-in on symbol 0, which stops out on candle 10, where symbol 2
    flags entry: with one slot and no other cash, symbol 2 enters on that
    candle with exactly the proceeds."""
    res, tr = _directed(1.0, [(0, 5), (2, 10)], [(2, 15)], 1,
                        lows=[(0, 10, 0.8)])
    assert res.refused.tolist() == [[0, 0]]
    assert tr["cash"][0, 5:10].tolist() == [0.0] * 5
    assert tr["n_open"][0, 9:16].tolist() == [1, 1, 1, 1, 1, 1, 0]
    keep = f32(1.0) - f32(FEE)
    units0 = f32(f32(1.0) * keep) / f32(1.0)
    proceeds = f32(f32(units0 * f32(0.875)) * keep)
    assert tr["cash"][0, 10] == 0.0           # all of it went to symbol 2
    units2 = f32(proceeds * keep) / f32(1.0)
    assert bits(tr["equity"][0, 10:11]) == bits(
        np.array([f32(0.0) + f32(units2 * f32(1.0))], f32))
    assert res.per_symbol[0, :, 0].tolist() == [1.0, 0.0, 1.0]
    assert res.per_symbol[0, 0, 3] > 0        # symbol 0's stop was a loss


def test_a_candidate_without_cash_is_refused_and_takes_no_slot():
    res, tr = _directed(1.0, [(0, 5), (1, 5)], [(0, 10), (1, 10)], 2)
    assert res.refused.tolist() == [[0, 1]]
    assert tr["n_open"][0, 4:11].tolist() == [0, 1, 1, 1, 1, 1, 0]
    assert res.per_symbol[0, :, 0].tolist() == [1.0, 0.0, 0.0]


def test_no_reentry_on_the_exit_candle():
    res, tr = _directed(0.5, [(0, 5), (0, 10)], [(0, 10)], 3)
    assert tr["n_open"][0, 9:13].tolist() == [1, 0, 0, 0]
    assert res.refused.tolist() == [[0, 0]]   # it was no candidate at all
    assert res.per_symbol[0, 0, 0] == 1.0


# ---------------------------------------------------------------------
# invariants on random flags
# ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 65, 1000, 2), (64, 5, 700, 1)])
def test_account_invariants(shape):
    nsym, P, T, max_positions = shape
    _c, _p, _e, _x, res, tr = pc.case_with_twin(shape)
    assert res.metrics[:, 1].sum() > 0
    assert (res.per_symbol[..., 0].sum(axis=1) == res.metrics[:, 1]).all()
    assert (res.per_symbol[..., 1].sum(axis=1) == res.metrics[:, 2]).all()
    assert (tr["cash"] >= 0).all()
    assert (tr["n_open"] >= 0).all()
    assert (tr["n_open"] <= max_positions).all()
    assert tr["n_open"].max() == max_positions
    assert (bits(res.equity) == bits(tr["equity"])).all()
    assert (bits(res.metrics[:, 0]) == bits(tr["equity"][:, -1])).all()


def test_gpu_cases_reach_every_branch():
    """The shapes test_gpu_portfolio.py runs, on the twin alone: each exits
    by stop, take-profit and flag and, where slots are scarce, refuses for
    slots; at least one refuses for cash."""
    assert all(T % 64 for _n, _P, T, _m in pc.CASES)
    assert max(pc.assert_reaches_every_branch(s) for s in pc.CASES) > 0


@pytest.mark.parametrize("stride", [7, 64, 5000])
def test_equity_samples_are_the_trace_at_the_sampled_candles(stride):
    shape = (3, 65, 1000, 2)
    candles, pop, ef, xf, full, tr = pc.case_with_twin(shape)
    res = run_portfolio_from_flags_cpu(
        candles, pop, ef, xf, max_positions=shape[3],
        initial_equity=pc.INITIAL_EQUITY, equity_stride=stride)
    assert res.equity.shape == (shape[1], -(-shape[2] // stride))
    assert (bits(res.equity) == bits(pc.strided(tr["equity"], stride))).all()
    assert (bits(res.equity[:, -1]) == bits(res.metrics[:, 0])).all()
    assert (bits(res.metrics) == bits(full.metrics)).all()


def test_bad_shapes_raise():
    candles = np.ones((65, 10, 4), f32)
    pop = random_population(2, seed=1)
    flags = np.zeros((2, 65, 10), bool)
    with pytest.raises(ValueError):
        run_portfolio_from_flags_cpu(candles, pop, flags, flags,
                                     max_positions=1)
    for bad in (0, 4):
        with pytest.raises(ValueError):
            run_portfolio_from_flags_cpu(
                candles[:3], pop, flags[:, :3], flags[:, :3],
                max_positions=bad)
    with pytest.raises(ValueError):
        run_portfolio_backtest_cpu(candles[:3], pop, max_positions=4)
