"""The trade ledger of the CPU twin (engine_cpu.run_backtest_cpu with
record_trades=True), and the engine / analyzer / CLI on top of it.

The twin is the reference the HIP ledger kernel is held to
(test_gpu_ledger.py), so these cases pin what a record means against the
candles, the parameters and the metrics the run itself reports.
"""

import csv
import json
import subprocess
import sys

import numpy as np
import pytest

from ledger_cases import (
    CAP, N_EAGER, NEVER, NSYM, SMALL_CAP, T_SHORT, assert_filler,
    assert_prefix, assert_sampled, short_inputs,
)

from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
from ai_crypto_trader_amd.backtesting.ledger import REASONS
from ai_crypto_trader_amd.backtesting.strategy import FEE, WARMUP

f32 = np.float32


@pytest.fixture(scope="module")
def case():
    mkt, pop = short_inputs()
    plain, curves = run_backtest_cpu(mkt, pop, record_equity=True)
    led = run_backtest_cpu(mkt, pop, record_trades=True, max_trades=CAP)
    for a in (plain, curves, led.metrics, led.n_records, led.equity):
        a.setflags(write=False)
    return mkt, pop, plain, curves, led


def test_metrics_unchanged(case):
    mkt, pop, plain, _, led = case
    np.testing.assert_array_equal(led.metrics, plain)
    np.testing.assert_array_equal(run_backtest_cpu(mkt, pop), plain)


def test_sharpness(case):
    """The inputs exercise every exit reason, an open position, a lane
    without trades, and fit the capacity."""
    _, _, _, _, led = case
    assert led.n_records.max() <= CAP
    kept = led.reason[led.reason >= 0]
    for r in range(1, 5):
        assert (kept == r).any(), REASONS[r]
    assert (kept == 0).any()                       # a lane ends open
    assert (led.n_records[NEVER] == 0).all()
    assert (led.n_records[:N_EAGER] > 0).all()
    assert_filler(led)


def test_record_invariants(case):
    mkt, pop, _, _, led = case
    close = mkt[:, :, 0]
    for p in range(pop.shape[0]):
        sl, tp = pop[p, 13], pop[p, 14]
        for s in range(NSYM):
            n = int(led.n_records[p, s])
            et, xt = led.entry_t[p, s, :n], led.exit_t[p, s, :n]
            why = led.reason[p, s, :n]
            n_open = int((why == 0).sum())
            assert n == int(led.metrics[p, s, 1]) + n_open
            assert n_open <= 1 and (why[:-1] != 0).all()
            closed = why != 0
            assert (et >= WARMUP).all()
            assert (xt[closed] > et[closed]).all()
            assert (xt[~closed] == -1).all()
            assert (et[1:] > xt[:-1]).all()
            ep, xp = led.entry_price[p, s, :n], led.exit_price[p, s, :n]
            np.testing.assert_array_equal(ep, close[s, et])
            np.testing.assert_array_equal(
                xp[why == 2], (ep * (f32(1.0) + tp))[why == 2])
            stop0 = ep * (f32(1.0) - sl)
            np.testing.assert_array_equal(xp[why == 1], stop0[why == 1])
            assert (xp[why == 4] > stop0[why == 4]).all()
            np.testing.assert_array_equal(
                xp[why == 3], close[s, xt[why == 3]])
            assert (xp[~closed] == 0).all()
            # units / cost / pnl tie together as the state machine did it
            units, cost = led.units[p, s, :n], led.entry_cost[p, s, :n]
            np.testing.assert_array_equal(
                units, cost * (f32(1.0) - f32(FEE)) / ep)
            pnl = led.pnl[p, s, :n]
            np.testing.assert_array_equal(
                pnl[closed],
                (units * xp * (f32(1.0) - f32(FEE)) - cost)[closed])
            assert (pnl[~closed] == 0).all()
            # f32 in-order replay of the metrics accumulator
            wins = gp = gl = f32(0.0)
            for x in pnl[closed]:
                wins = wins + f32(x > 0)
                gp = gp + np.maximum(x, f32(0.0))
                gl = gl + np.maximum(-x, f32(0.0))
            assert wins == led.metrics[p, s, 2]
            assert gp == led.metrics[p, s, 3]
            assert gl == led.metrics[p, s, 4]


def test_capacity(case):
    mkt, pop, _, _, led = case
    small = run_backtest_cpu(mkt, pop, record_trades=True,
                             max_trades=SMALL_CAP)
    assert_prefix(small, led)


def test_equity_stride_one_is_the_curve(case):
    _, _, _, curves, led = case
    assert led.equity_stride == 1
    np.testing.assert_array_equal(led.equity, curves)
    assert_sampled(led, curves, T_SHORT)


@pytest.mark.parametrize("stride", [7, 256])
def test_equity_stride(case, stride):
    mkt, pop, _, curves, _ = case
    led = run_backtest_cpu(mkt, pop, record_trades=True, max_trades=CAP,
                           equity_stride=stride)
    assert_sampled(led, curves, T_SHORT)


def test_trades_dicts_feed_the_evaluation(case):
    from ai_crypto_trader_amd.backtesting.evaluation import (
        calculate_advanced_metrics, calculate_metrics,
    )
    _, _, _, _, led = case
    trades = led.trades(0, 0)
    assert len(trades) == led.n_records[0, 0]
    t = trades[0]
    assert t["reason"] in REASONS and isinstance(t["pnl"], float)
    assert t["duration"] == t["exit_t"] - t["entry_t"]
    closed = [t for t in trades if t["reason"] != "open"]
    m = calculate_metrics(led.equity[0, 0], closed)
    assert m["n_trades"] == led.metrics[0, 0, 1]
    assert m["win_rate"] == led.metrics[0, 0, 2] / led.metrics[0, 0, 1]
    assert "expectancy" in calculate_advanced_metrics(led.equity[0, 0],
                                                      closed)
    assert led.trades(NEVER, 0) == []


# --- engine, analyzer, CLI on device="cpu" -------------------------------

EAGER = {"entry_votes": 1, "exit_votes": 1, "stop_loss_pct": 0.004,
         "take_profit_pct": 0.006, "trailing_stop_pct": 0.003,
         "trailing_act_pct": 0.002}


@pytest.fixture(scope="module")
def engine_stats(tmp_path_factory):
    from ai_crypto_trader_amd.backtesting.engine import BacktestEngine
    d = tmp_path_factory.mktemp("ledger_engine")
    eng = BacktestEngine(str(d), device="cpu")
    stats = eng.run_backtest("BTCUSDC", "default", n_candles=3000,
                             params=EAGER, record_trades=True,
                             record_equity=True, equity_stride=60)
    return d, eng, stats


def test_engine_stats(engine_stats):
    _, eng, stats = engine_stats
    assert stats["n_trades"] > 5
    assert len(stats["trades"]) == stats["n_trades"] + stats["n_open"]
    assert stats["n_records"] == len(stats["trades"])
    assert len(stats["equity_curve"]) == 3000 // 60
    assert stats["equity_curve"][-1] == stats["final_equity"]
    for k in ("avg_win", "avg_loss", "max_win_streak", "max_loss_streak",
              "expectancy"):
        assert k in stats
    saved = json.loads(eng.last_saved.read_text())
    assert saved["trades"] == stats["trades"]
    assert "equity_curve" not in saved
    # capacity reaches the engine
    few = eng.run_backtest("BTCUSDC", "default", n_candles=3000,
                           params=EAGER, record_trades=True, max_trades=3)
    assert few["trades"] == stats["trades"][:3]
    assert few["n_records"] == stats["n_records"]
    with pytest.raises(ValueError):
        eng.run_backtest("BTCUSDC", "grid", n_candles=3000,
                         record_trades=True)


def test_trade_analysis(engine_stats):
    from ai_crypto_trader_amd.backtesting.result_analyzer import (
        ResultAnalyzer,
    )
    d, _, stats = engine_stats
    ra = ResultAnalyzer(str(d / "analysis"))
    plain = ra.trade_analysis({k: v for k, v in stats.items()
                               if k != "trades"})
    ta = ra.trade_analysis(stats)
    assert set(plain) < set(ta)
    assert {k: ta[k] for k in plain} == plain
    closed = [t for t in stats["trades"] if t["reason"] != "open"]
    assert sum(r["count"] for r in ta["by_reason"].values()) \
        == len(closed) == stats["n_trades"]
    realized = sum(t["pnl"] for t in closed)
    assert sum(r["pnl"] for r in ta["by_reason"].values()) \
        == pytest.approx(realized, rel=1e-9)
    assert ta["expectancy"] == pytest.approx(realized / len(closed))
    assert ta["median_duration"] > 0 and ta["mean_duration"] > 0
    p = ra.plot_trade_analysis(stats)
    assert p.suffix == ".png" and p.stat().st_size > 1000


def test_cli_writes_the_csv(engine_stats, tmp_path):
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run(
        [sys.executable, str(root / "run_backtest.py"), "--data-dir",
         str(tmp_path), "backtest", "--symbol", "BTCUSDC", "--cpu",
         "--candles", "3000", "--params", json.dumps(EAGER), "--trades",
         "--max-trades", "64", "--equity-stride", "60", "--plot"],
        capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "trailing_stop" in r.stdout and "take_profit" in r.stdout
    (saved,) = (tmp_path / "results").glob("*.json")
    (out,) = (tmp_path / "results").glob("*_trades.csv")
    assert out.name == saved.stem + "_trades.csv"
    with open(out) as f:
        rows = list(csv.DictReader(f))
    trades = json.loads(saved.read_text())["trades"]
    assert len(rows) == len(trades) > 0
    assert rows[0]["reason"] == trades[0]["reason"]
    assert int(rows[0]["entry_t"]) == trades[0]["entry_t"]
    assert (tmp_path / "analysis" / "BTCUSDC_trades.png").exists()
