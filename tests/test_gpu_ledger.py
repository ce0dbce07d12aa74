"""backtest_ledger_kernel (ops/hip/backtest_ledger.hip) vs its CPU twin.

Every field of every record, the record counts, the equity samples and
the metrics are held to bit equality with
engine_cpu.run_backtest_cpu(record_trades=True): the project already
demands CPU<->GPU bit equality of the metrics (test_gpu_continuous.py), and
a record is made of the same f32 values. The cases aim at what the
recorder can get wrong: a partial block, the plain block map, a history
that ends inside a tile, a lane without trades, capacity overflow, the
strided equity counter and its last sample, independence from which
strategies share a block, and the peeled resnap candle.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ledger_cases import (  # noqa: E402
    CAP, NEVER, SMALL_CAP, T_SHORT, assert_filler, assert_ledgers_equal,
    assert_prefix, assert_sampled, eager_population, market, short_inputs,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gpu(dev, mkt, pop, **kw):
    from ai_crypto_trader_amd.ops.backtest import run_backtest_ledger_gpu
    led = run_backtest_ledger_gpu(torch.from_numpy(mkt).to(dev),
                                  torch.from_numpy(pop).to(dev), **kw)
    torch.cuda.synchronize()
    return led.numpy()


@pytest.fixture(scope="module")
def short_case(dev):
    """T=700 x 3 symbols x 41 strategies, max_trades=128, stride 1: the
    twin's ledger (computed once, read-only) and the GPU's."""
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    mkt, pop = short_inputs()
    ref = run_backtest_cpu(mkt, pop, record_trades=True, max_trades=CAP)
    for a in (ref.metrics, ref.n_records, ref.equity, ref.entry_t,
              ref.exit_t, ref.reason, ref.entry_price, ref.exit_price,
              ref.units, ref.entry_cost, ref.pnl):
        a.setflags(write=False)
    return mkt, pop, ref, _gpu(dev, mkt, pop, max_trades=CAP)


def test_equal_to_the_twin(short_case):
    _, _, ref, got = short_case
    assert ref.n_records.max() <= CAP and ref.n_records.max() > SMALL_CAP
    assert (ref.reason == 0).any()                 # an open position
    assert_ledgers_equal(got, ref)
    assert (got.n_records[NEVER] == 0).all()
    assert_filler(got)


def test_metrics_equal_the_headline_kernel(dev, short_case):
    from ai_crypto_trader_amd.ops.backtest import run_backtest_gpu
    mkt, pop, _, got = short_case
    m = run_backtest_gpu(torch.from_numpy(mkt).to(dev),
                         torch.from_numpy(pop).to(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.metrics, m.cpu().numpy())


@pytest.mark.parametrize("stride", [7, 256])
def test_overflow_and_stride(dev, short_case, stride):
    """max_trades=16 overflows most lanes and not all; the samples are
    the twin's stride-1 curve at the defined candles."""
    mkt, pop, ref, _ = short_case
    got = _gpu(dev, mkt, pop, max_trades=SMALL_CAP, equity_stride=stride)
    assert_prefix(got, ref)
    assert_sampled(got, ref.equity, T_SHORT)


def test_launch_independence(dev, short_case):
    """P=300: one full 256 block and one with 44 active lanes. The launch
    equals its first 256 and last 44 rows launched separately."""
    mkt = short_case[0]
    pop = eager_population(300, seed=17)
    kw = dict(max_trades=CAP, equity_stride=64)
    got = _gpu(dev, mkt, pop, **kw)
    assert got.n_records.max() <= CAP and got.n_records.min() > 0
    head = _gpu(dev, mkt, np.ascontiguousarray(pop[:256]), **kw)
    tail = _gpu(dev, mkt, np.ascontiguousarray(pop[256:]), **kw)
    for f in ("metrics", "n_records", "entry_t", "exit_t", "reason",
              "entry_price", "exit_price", "units", "entry_cost", "pnl",
              "equity"):
        a = getattr(got, f)
        np.testing.assert_array_equal(a[:256], getattr(head, f), err_msg=f)
        np.testing.assert_array_equal(a[256:], getattr(tail, f), err_msg=f)
    assert_filler(got)
    assert got.equity.shape[-1] == -(-T_SHORT // 64)
    np.testing.assert_array_equal(got.equity[..., -1], got.metrics[..., 0])


def test_resnap_boundary(dev):
    """T = RESNAP + 600, one symbol, 8 strategies, max_trades=2048,
    stride 1440: thousands of records per lane across the resnap tile."""
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    from ai_crypto_trader_amd.backtesting.strategy import RESNAP
    T = RESNAP + 600
    mkt = market(T, 1, seed=5)
    pop = eager_population(8, seed=3)
    kw = dict(max_trades=2048, equity_stride=1440)
    ref = run_backtest_cpu(mkt, pop, record_trades=True, **kw)
    got = _gpu(dev, mkt, pop, **kw)
    assert ref.n_records.max() <= 2048 and ref.n_records.max() > 500
    assert (ref.exit_t > RESNAP).any()
    assert_ledgers_equal(got, ref)
    assert got.equity.shape[-1] == -(-T // 1440)


def test_engine_cuda_equals_cpu(tmp_path):
    from ai_crypto_trader_amd.backtesting.engine import BacktestEngine
    params = {"entry_votes": 1, "exit_votes": 1, "stop_loss_pct": 0.004,
              "take_profit_pct": 0.006, "trailing_stop_pct": 0.003,
              "trailing_act_pct": 0.002}
    out = {}
    for device in ("cpu", "cuda"):
        eng = BacktestEngine(str(tmp_path / device), device=device)
        out[device] = eng.run_backtest(
            "BTCUSDC", "default", n_candles=3000, params=params,
            record_trades=True, record_equity=True, equity_stride=60)
    cpu, gpu = out["cpu"], out["cuda"]
    assert gpu["engine"] == "cuda" and len(cpu["trades"]) > 5
    assert gpu["trades"] == cpu["trades"]
    assert gpu["equity_curve"] == cpu["equity_curve"]
    for k in ("n_trades", "n_open", "n_records", "expectancy", "avg_win",
              "avg_loss", "max_win_streak", "max_loss_streak"):
        assert gpu[k] == cpu[k], k
