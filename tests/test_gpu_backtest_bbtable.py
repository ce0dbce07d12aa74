"""backtest_kernel's block-shared Bollinger table vs the CPU engine.

31 lanes of every block march the f64 Bollinger sums, one window length
each, the block turns them into an LDS table of {mean, std}, and every
lane reads its window's entry. These cases aim at what that can get
wrong: every window value and the clamp, blocks whose scan lanes hold no
active strategy, the plain block map, histories that end inside a table
sub-tile, the resnap tile, and independence from which strategies share a
block.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

T_SHORT = 700        # 2 tiles of 256 + 188 = 5 table sub-tiles of 32 + 28
NSYM = 3             # not a multiple of 8: the non-XCD-affine block map


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _market(T, nsym, seed):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(T, nsym, seed=seed, sigma=2.0))


def _windows_population(P, seed):
    """Random strategies whose bb_window slot cycles through every value
    2..32 and three inputs the kernel has to clamp/truncate (1.0 -> 2,
    4.7 -> 4, 40.0 -> 32); eager entry/exit votes so the Bollinger vote
    decides trades."""
    from ai_crypto_trader_amd.backtesting.strategy import random_population
    pop = random_population(P, seed=seed)
    wins = np.array(list(range(2, 33)) + [1.0, 4.7, 40.0], dtype=np.float32)
    # stride 7 is coprime to 34: neighbours differ, every 64-lane wave of
    # a 256 block sees many windows, and each window recurs every 34 lanes
    pop[:, 6] = wins[(np.arange(P) * 7) % len(wins)]
    pop[:, 10] = 1.0 + (np.arange(P) % 2)      # entry_votes 1/2
    pop[:, 11] = 1.0 + ((np.arange(P) // 2) % 2)
    return pop


def _gpu(dev, market, pop):
    from ai_crypto_trader_amd.ops.backtest import run_backtest_gpu
    got = run_backtest_gpu(torch.from_numpy(market).to(dev),
                           torch.from_numpy(pop).to(dev))
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _assert_parity(got, ref):
    np.testing.assert_array_equal(got[..., 1], ref[..., 1])   # n_trades
    np.testing.assert_array_equal(got[..., 2], ref[..., 2])   # wins
    np.testing.assert_allclose(got[..., 0], ref[..., 0], rtol=2e-5)
    np.testing.assert_allclose(got[..., 5], ref[..., 5], rtol=1e-3,
                               atol=1e-6)
    np.testing.assert_allclose(got[..., 9], ref[..., 9], rtol=1e-3,
                               atol=1e-3)


@pytest.fixture(scope="module")
def short_case(dev):
    """T=700 x 3 symbols x 300 strategies: CPU reference and the single
    GPU launch, computed once."""
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    market = _market(T_SHORT, NSYM, seed=31)
    pop = _windows_population(300, seed=17)
    assert set(np.clip(pop[:, 6].astype(np.int32), 2, 32)) == set(
        range(2, 33))
    ref = run_backtest_cpu(market, pop)
    ref.setflags(write=False)
    got = _gpu(dev, market, pop)
    return market, pop, ref, got


def test_every_window_partial_chunk(short_case):
    """P=300: one full 256 block and one with 44 active lanes, three of
    whose four waves hold no strategy at all."""
    _, _, ref, got = short_case
    assert ref[..., 1].sum() > 0                  # trades happen at all
    _assert_parity(got, ref)


def test_bollinger_vote_matters(short_case):
    """The cases above are only sharp if the table's values decide
    trades: shifting every window by one changes the CPU trade counts."""
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    market, pop, ref, _ = short_case
    other = pop.copy()
    other[:, 6] = np.where(np.clip(pop[:, 6], 2, 32) >= 32, 31.0,
                           np.floor(np.clip(pop[:, 6], 2, 32)) + 1.0)
    alt = run_backtest_cpu(market, other)
    assert (alt[..., 1] != ref[..., 1]).any()


def test_fewer_strategies_than_scan_lanes(dev, short_case):
    """P=40: barely more strategies than the 31 scan lanes, and far fewer
    than the lanes that convert the table."""
    market, pop, ref, _ = short_case
    got = _gpu(dev, market, np.ascontiguousarray(pop[:40]))
    _assert_parity(got, ref[:40])


def test_launch_independence(dev, short_case):
    """The table must not depend on which strategies share a block: the
    300-strategy launch equals its first 256 and last 44 rows launched
    separately, bit for bit."""
    market, pop, _, got = short_case
    head = _gpu(dev, market, np.ascontiguousarray(pop[:256]))
    tail = _gpu(dev, market, np.ascontiguousarray(pop[256:]))
    assert np.array_equal(got[:256], head)
    assert np.array_equal(got[256:], tail)


def test_resnap_boundary(dev):
    """T = RESNAP + 600, one symbol, 64 strategies: the scan lanes
    recompute their sums at the resnap tile and skip that candle's
    increment."""
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    from ai_crypto_trader_amd.backtesting.strategy import RESNAP
    T = RESNAP + 600
    market = _market(T, 1, seed=5)
    pop = _windows_population(64, seed=3)
    ref = run_backtest_cpu(market, pop)
    got = _gpu(dev, market, pop)
    _assert_parity(got, ref)
    head = run_backtest_cpu(np.ascontiguousarray(market[:, :RESNAP]), pop)
    assert (ref[..., 1] > head[..., 1]).any()     # trades after the resnap
