"""backtest_kernel's shortened lane loop computes what it computed before.

The loop lost instructions the result does not need: max/min without the
self-max canonicalisation, EMAs seeded with close[0] instead of a t == 0
select, one LDS record {close, high, low, change | shared votes} per
candle, the trailing trigger computed at entry, and a recurrence-only loop
for the warm-up sub-tiles. Each case is held three ways:

  - bit for bit against tests/golden/backtest_lane_loop.npz, which the
    build of the commit BEFORE that change wrote on a GPU
    (tools/make_backtest_golden.py; never regenerate it from the code
    under test) — all 10 metrics, column for column;
  - against engine_cpu.run_backtest_cpu: trade counts and wins exactly,
    equity/drawdown/fitness at test_gpu_backtest_bbtable's tolerances;
  - bit for bit against run_backtest_continuous_gpu(nshards=1), whose
    flags kernel keeps the unseeded t == 0 form and its own LDS layout.

The golden holds outputs only; the inputs are rebuilt from the seeds in
tools/make_backtest_golden.py.
"""

import functools
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tools import make_backtest_golden as gen  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "backtest_lane_loop.npz"
METRICS = ("equity", "n_trades", "wins", "gross_p", "gross_l", "max_dd",
           "sum_ret", "sum_ret2", "sharpe", "fitness")


@functools.lru_cache(maxsize=None)
def _cases():
    return gen.cases()


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _cpu(name):
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    ref = run_backtest_cpu(*_cases()[name])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _gpu(name):
    from ai_crypto_trader_amd.ops.backtest import run_backtest_gpu
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    market, pop = _cases()[name]
    got = run_backtest_gpu(torch.from_numpy(market).to(dev),
                           torch.from_numpy(pop).to(dev))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    got.setflags(write=False)
    return got


def _continuous(name):
    from ai_crypto_trader_amd.ops.backtest import run_backtest_continuous_gpu
    dev = torch.device("cuda:0")
    market, pop = _cases()[name]
    got = run_backtest_continuous_gpu(torch.from_numpy(market).to(dev),
                                      torch.from_numpy(pop).to(dev),
                                      nshards=1)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _assert_golden(name):
    got, want = _gpu(name), _golden()[name]
    assert got.shape == want.shape and got.dtype == want.dtype
    for k, metric in enumerate(METRICS):
        assert np.array_equal(got[..., k], want[..., k]), (
            f"{name}: {metric} differs from the parent kernel in "
            f"{(got[..., k] != want[..., k]).sum()} of {want[..., k].size}")


def _assert_cpu(name):
    # the tolerances of test_gpu_backtest_bbtable._assert_parity
    got, ref = _gpu(name), _cpu(name)
    np.testing.assert_array_equal(got[..., 1], ref[..., 1])   # n_trades
    np.testing.assert_array_equal(got[..., 2], ref[..., 2])   # wins
    np.testing.assert_allclose(got[..., 0], ref[..., 0], rtol=2e-5)
    np.testing.assert_allclose(got[..., 5], ref[..., 5], rtol=1e-3,
                               atol=1e-6)
    np.testing.assert_allclose(got[..., 9], ref[..., 9], rtol=1e-3,
                               atol=1e-3)


def _assert_three_ways(name):
    _assert_golden(name)
    _assert_cpu(name)
    assert np.array_equal(_gpu(name), _continuous(name))


def test_golden_file_is_complete():
    want = {f"T{T}" for T in gen.T_CASES} | {"trailing", "resnap"}
    assert set(_golden()) == want
    for name, (market, pop) in _cases().items():
        assert _golden()[name].shape == (len(pop), len(market), len(METRICS))


def test_symbols_differ_by_orders_of_magnitude():
    market, _ = _cases()["T700"]
    lvl = market[:, 0, 0]
    assert lvl[1] > 30 * lvl[0] and lvl[0] > 90 * lvl[2]


@pytest.mark.parametrize("T", gen.T_CASES)
def test_history_length(T):
    """nsym = 3, P = 70 (one full wave and a 6-lane wave): a single
    candle, both sides of the warm-up boundary, the first voting candle,
    sub-tile remainders after a tile boundary, a ragged last sub-tile."""
    name = f"T{T}"
    market, pop = _cases()[name]
    assert market.shape == (gen.NSYM, T, 4) and len(pop) == gen.P_LANES
    if T == 700:
        assert (_cpu(name)[..., 1].sum(axis=0) > 0).all()   # every symbol
    _assert_three_ways(name)


def test_trailing_stop():
    """Even lanes trail with a trigger that fires; odd lanes have the
    trailing stop off. Sharp only if trailing decides trades: zeroing
    trailing_stop_pct changes the CPU result on the trailing lanes."""
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    market, pop = _cases()["trailing"]
    assert market.shape[1] == 700 and len(pop) == 64
    even = (np.arange(len(pop)) % 2) == 0
    assert (pop[even, 15] > 0).all() and (pop[~even, 15] == 0).all()
    ref = _cpu("trailing")
    off = pop.copy()
    off[:, 15] = 0.0
    alt = run_backtest_cpu(market, off)
    assert ((alt[even][..., 1] != ref[even][..., 1])
            | (alt[even][..., 0] != ref[even][..., 0])).any(axis=1).all()
    assert np.array_equal(alt[~even], ref[~even])
    _assert_three_ways("trailing")


def test_resnap_instantiation():
    """T = RESNAP + 600 runs backtest_kernel<true>: golden equality plus
    the CPU checks."""
    from ai_crypto_trader_amd.backtesting.strategy import RESNAP
    market, pop = _cases()["resnap"]
    assert market.shape == (1, RESNAP + 600, 4) and len(pop) == 64
    _assert_golden("resnap")
    _assert_cpu("resnap")
