"""Fill ledgers of the grid and DCA families on the CPU: the numpy twins'
records against fill lists worked out by hand from the contracts in
strategy_grid.py / strategy_dca.py, the ledger's accounting identities on a
volatile random market, capacity, equity strides, round trips, and the
plumbing through BacktestEngine, the CLI and ResultAnalyzer."""

import csv
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ai_crypto_trader_amd.backtesting.engine_dca_cpu import (
    run_dca_backtest_cpu,
)
from ai_crypto_trader_amd.backtesting.engine_grid_cpu import (
    run_grid_backtest_cpu,
)
from ai_crypto_trader_amd.backtesting.families import FAMILIES
from ai_crypto_trader_amd.backtesting.fills import (
    DEFAULT_MAX_FILLS, FIELDS, FILL_KINDS, FLOAT_FIELDS, INT_FIELDS,
    KIND_BUILD, FillLedger,
)
from ai_crypto_trader_amd.backtesting.ledger import n_equity_samples

REPO = Path(__file__).resolve().parent.parent
FEE = 0.001
OMF = 1.0 - FEE
f32 = np.float32


def series(rows):
    """[(close, high, low), ...] -> (1, T, 4) candles."""
    a = np.array([(c, h, lo, 1.0) for c, h, lo in rows], np.float32)
    return a[None]


def check_fills(got, want):
    """got: FillLedger.fills(); want: [(t, kind, slot, price, units, cash,
    pnl, units_held), ...] — integers and names exactly, floats to f32
    rounding of the hand arithmetic (which is in f64)."""
    assert [(f["t"], f["kind"], f["slot"]) for f in got] \
        == [w[:3] for w in want]
    for f, w in zip(got, want):
        for name, v in zip(FLOAT_FIELDS, w[3:]):
            assert f[name] == pytest.approx(v, rel=2e-6, abs=1e-7), \
                (f["t"], f["kind"], f["slot"], name)


def test_layout():
    assert FILL_KINDS == ("buy", "sell", "build", "breakout", "scheduled",
                          "dip", "scheduled_dip", "take_profit")
    assert FIELDS == ("t", "kind", "slot", "price", "units", "cash", "pnl",
                      "units_held")
    assert INT_FIELDS == FIELDS[:3] and len(FIELDS) * 4 == 32
    assert DEFAULT_MAX_FILLS >= 4096


# --- grid, by hand --------------------------------------------------------

def test_grid_h2_fill_list_by_hand():
    # H=2, s=0.1 %, arithmetic, all equity committed, 5 % breakout band:
    # levels 0.998 0.999 1.000 1.001 1.002 around close[0] = 1, b = 1/4.
    # A step smaller than two fees makes every round trip lose a little,
    # which is what lets cash fall below b.
    p = np.array([[2, 0.001, 0, 1.0, 0.05]], np.float32)
    rows = [
        (1.0, 1.0, 1.0),         # t0 build: slots 2, 3 at market
        (1.0, 1.002, 1.0),       # t1 high reaches L[3], L[4]: sell 2 then 3
        (1.0005, 1.0005, 1.0),   # t2 low reaches L[3], L[2]: buy 3 then 2
        (0.998, 1.0, 0.998),     # t3 low reaches L[1], L[0]: buy 1; then
                                 #    cash 0.24975 < b stops slot 0
        (0.94, 0.998, 0.94),     # t4 close < L[0]*0.95: still no cash for
                                 #    slot 0; liquidate 1, 2, 3; rebuild
    ]
    led = run_grid_backtest_cpu(series(rows), p, record_fills=True)
    b = 0.25
    u0 = b * OMF / 1.0
    s2 = u0 * 1.001 * OMF               # proceeds of slot 2 at L[3]
    s3 = u0 * 1.002 * OMF               # of slot 3 at L[4]
    u3 = b * OMF / 1.001                # rebuy of slot 3 at L[3]
    u2 = b * OMF / 1.000
    u1 = b * OMF / 0.999
    held = u3 + u2 + u1
    x1, x2, x3 = (u * 0.94 * OMF for u in (u1, u2, u3))
    cash = 1.0 - 2 * b + s2 + s3 - 3 * b + x1 + x2 + x3
    b2 = cash / 4
    v0 = b2 * OMF / 0.94
    want = [
        (0, "build", 2, 1.0, u0, -b, 0.0, u0),
        (0, "build", 3, 1.0, u0, -b, 0.0, 2 * u0),
        (1, "sell", 2, 1.001, u0, s2, s2 - b, u0),
        (1, "sell", 3, 1.002, u0, s3, s3 - b, 0.0),
        (2, "buy", 3, 1.001, u3, -b, 0.0, u3),
        (2, "buy", 2, 1.000, u2, -b, 0.0, u3 + u2),
        (3, "buy", 1, 0.999, u1, -b, 0.0, held),
        # the liquidation does not touch units_total (fills.py)
        (4, "breakout", 1, 0.94, u1, x1, x1 - b, held),
        (4, "breakout", 2, 0.94, u2, x2, x2 - b, held),
        (4, "breakout", 3, 0.94, u3, x3, x3 - b, held),
        (4, "build", 2, 0.94, v0, -b2, 0.0, v0),
        (4, "build", 3, 0.94, v0, -b2, 0.0, 2 * v0),
    ]
    assert s2 - b < 0 and s3 - b < 0    # the premise of t3
    assert led.n_records[0, 0] == len(want)
    check_fills(led.fills(0, 0), want)
    assert led.metrics[0, 0, 1] == 5 and led.metrics[0, 0, 2] == 0
    trips = led.round_trips(0, 0)
    # closed in closing order, each paired with the fill that last filled
    # its slot (t0 builds; t3 buy of 1; t2 buys of 2 and 3); then the two
    # slots the rebuild holds
    assert [(t["entry_t"], t["exit_t"], t["reason"]) for t in trips] == [
        (0, 1, "sell"), (0, 1, "sell"), (3, 4, "breakout"),
        (2, 4, "breakout"), (2, 4, "breakout"), (4, -1, "open"),
        (4, -1, "open")]
    assert trips[3]["entry_price"] == pytest.approx(1.0)
    assert trips[4]["entry_price"] == pytest.approx(1.001)
    assert trips[5]["entry_cost"] == pytest.approx(b2, rel=2e-6)
    assert trips[5]["pnl"] == 0.0 and trips[5]["exit_price"] == 0.0


def test_grid_h16_geometric_by_hand():
    # H=16, geometric 0.5 % steps, half the equity committed: b = 0.5/32.
    # t1's high reaches L[19] = 1.005^3 but not L[20]: slots 16, 17, 18
    # (sell prices L[17], L[18], L[19]) sell, ascending
    p = np.array([[16, 0.005, 1, 0.5, 0.5]], np.float32)
    r = 1.005
    rows = [(1.0, 1.0, 1.0), (1.01, r ** 3 + 1e-4, 1.0)]
    led = run_grid_backtest_cpu(series(rows), p, record_fills=True)
    b = 0.5 / 32
    u0 = b * OMF
    want = [(0, "build", 15 + j, 1.0, u0, -b, 0.0, j * u0)
            for j in range(1, 17)]
    for i in range(3):
        px = r ** (i + 1)
        want.append((1, "sell", 16 + i, px, u0, u0 * px * OMF,
                     u0 * px * OMF - b, (15 - i) * u0))
    check_fills(led.fills(0, 0), want)
    # the last build fill's running count IS (float)units_total
    assert led.units_held[0, 0, 15] == f32(np.float64(16) * np.float64(
        led.units[0, 0, 15]))
    assert len(led.round_trips(0, 0)) == 3 + 13


# --- DCA, by hand ---------------------------------------------------------

def test_dca_fill_list_by_hand():
    # period 4, base 1 % of equity, dip threshold 10 % (x2, cooldown 3),
    # take profit 5 %, value averaging on
    p = np.array([[4, 0.01, 0.1, 2.0, 3, 0.05, 1]], np.float32)
    flat, mid, low = (1.0, 1.0, 1.0), (0.95, 0.95, 0.95), (0.85, 0.85, 0.85)
    rows = ([flat] * 7            # t3: scheduled, n/period = 1
            + [mid] * 4           # t7: scheduled, value-averaged, n/p = 2
            + [low] * 5           # t11: scheduled AND dip; t14: dip alone
                                  # (cooldown over); t15: schedule wants 0
            + [(0.93, 0.94, 0.85)]   # t16: high reaches tp_price
            + [flat] * 4)         # t20: first buy of cycle 1
    led = run_dca_backtest_cpu(series(rows), p, record_fills=True)
    base = 0.01
    usd0 = base * 1 - 0.0
    d0 = usd0 * OMF / 1.0
    usd1 = base * 2 - d0 * 0.95             # value averaging: the gap
    d1 = usd1 * OMF / 0.95
    usd2 = (base * 3 - (d0 + d1) * 0.85) * 2.0      # gap, times dip_mult
    d2 = usd2 * OMF / 0.85
    usd3 = base * 2.0                       # dip alone: base * dip_mult
    d3 = usd3 * OMF / 0.85
    units = d0 + d1 + d2 + d3
    invested = usd0 + usd1 + usd2 + usd3
    assert base * 4 - units * 0.85 < 0      # t15: nothing to average in
    tp = invested / units * 1.05
    assert 0.85 < tp < 0.94
    proceeds = units * tp * OMF
    want = [
        (3, "scheduled", 0, 1.0, d0, -usd0, 0.0, d0),
        (7, "scheduled", 0, 0.95, d1, -usd1, 0.0, d0 + d1),
        (11, "scheduled_dip", 0, 0.85, d2, -usd2, 0.0, d0 + d1 + d2),
        (14, "dip", 0, 0.85, d3, -usd3, 0.0, units),
        (16, "take_profit", 0, tp, units, proceeds, proceeds - invested,
         0.0),
        (20, "scheduled", 1, 1.0, d0, -usd0, 0.0, d0),
    ]
    assert led.n_records[0, 0] == len(want)
    check_fills(led.fills(0, 0), want)
    trips = led.round_trips(0, 0)
    assert [(t["entry_t"], t["exit_t"], t["reason"]) for t in trips] == [
        (3, 16, "take_profit"), (20, -1, "open")]
    assert trips[0]["entry_cost"] == pytest.approx(invested, rel=2e-6)
    assert trips[0]["entry_price"] == pytest.approx(invested / units,
                                                    rel=2e-6)
    assert trips[0]["pnl"] == led.pnl[0, 0, 4]
    assert trips[1]["entry_cost"] == pytest.approx(usd0, rel=2e-6)
    assert trips[1]["units"] == pytest.approx(d0, rel=2e-6)


# --- a volatile random market ---------------------------------------------

P = 41


@pytest.fixture(scope="module")
def market():
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(700, 3, seed=7, sigma=3.0))


@pytest.fixture(scope="module", params=["grid", "dca"])
def run(request, market):
    """family, population, plain metrics, and the uncapped stride-1
    ledger: computed once, read by every test below."""
    fam = FAMILIES[request.param]
    pop = fam.random_population(P, 11)
    plain = fam.run_cpu(market, pop)
    n = fam.run_cpu_fills(market, pop, max_fills=1).n_records
    full = fam.run_cpu_fills(market, pop, max_fills=int(n.max()))
    return fam, pop, plain, full


def replay_equity(led, p, s, last_close, initial_equity=1.0):
    """The lane's final equity from its records alone, in the engines' own
    f32 operations and order. A (re)build takes its cash in one operation,
    cash - (float)H * b (fills.py), so a candle's build records are
    subtracted as that one product."""
    n = led.n_kept(p, s)
    cash = f32(initial_equity)
    k = 0
    while k < n:
        if led.kind[p, s, k] == KIND_BUILD:
            h = 1
            while (k + h < n and led.kind[p, s, k + h] == KIND_BUILD
                   and led.t[p, s, k + h] == led.t[p, s, k]):
                h += 1
            cash = f32(cash - f32(h) * f32(-led.cash[p, s, k]))
            k += h
        else:
            cash = f32(cash + led.cash[p, s, k])
            k += 1
    held = led.units_held[p, s, n - 1] if n else f32(0.0)
    return f32(cash + f32(held * last_close))


def test_random_market_accounting(run, market):
    fam, pop, plain, led = run
    assert led.n_records.max() <= led.max_fills
    np.testing.assert_array_equal(led.metrics, plain)
    closing = ((1, 3) if fam.name == "grid" else (7,))
    nsym = market.shape[0]
    for p in range(P):
        for s in range(nsym):
            n = led.n_kept(p, s)
            kind = led.kind[p, s, :n]
            closes = np.isin(kind, closing)
            assert closes.sum() == led.metrics[p, s, 1], (p, s)
            assert (closes & (led.pnl[p, s, :n] > 0)).sum() \
                == led.metrics[p, s, 2], (p, s)
            assert not led.pnl[p, s, :n][~closes].any()
            assert (np.diff(led.t[p, s, :n]) >= 0).all()
            assert replay_equity(led, p, s, market[s, -1, 0]) \
                == led.metrics[p, s, 0], (p, s)
    if fam.name == "grid":
        # non-vacuous: the shapes the issue measured
        assert led.metrics[..., 1].min() >= 27
        assert led.metrics[..., 1].max() >= 1000
        assert set(np.unique(led.kind[led.kind >= 0])) == {0, 1, 2, 3}
    else:
        assert (led.metrics[..., 1] > 0).sum() >= 20
        assert {4, 5, 7} <= set(np.unique(led.kind[led.kind >= 0]))
        # at most one record per candle
        for p in range(P):
            for s in range(nsym):
                n = led.n_kept(p, s)
                assert (np.diff(led.t[p, s, :n]) > 0).all()


def test_overflow_keeps_a_prefix(run, market):
    fam, pop, _, full = run
    n = np.sort(full.n_records.ravel())
    cap = max(int(n[len(n) // 4]), 1)       # three lanes in four overflow
    over = full.n_records > cap
    assert 0.5 < over.mean() < 1.0
    led = fam.run_cpu_fills(market, pop, max_fills=cap)
    assert led.max_fills == cap
    np.testing.assert_array_equal(led.n_records, full.n_records)
    np.testing.assert_array_equal(led.metrics, full.metrics)
    np.testing.assert_array_equal(led.equity, full.equity)
    kept = np.minimum(full.n_records, cap)[..., None] > np.arange(cap)
    for f in FIELDS:
        a = getattr(led, f)
        np.testing.assert_array_equal(a[kept], getattr(full, f)[..., :cap][
            kept], err_msg=f)
        assert (a[~kept] == (-1 if f in INT_FIELDS else 0)).all(), f
    p, s = np.argwhere(over)[0]
    with pytest.raises(ValueError, match="max_fills"):
        led.round_trips(p, s)
    p, s = np.argwhere(~over)[0]
    assert led.round_trips(p, s) == full.round_trips(p, s)


@pytest.mark.parametrize("stride", [7, 256])
def test_equity_stride(run, market, stride):
    fam, pop, _, full = run
    T = market.shape[1]
    led = fam.run_cpu_fills(market, pop, max_fills=8, equity_stride=stride)
    ns = n_equity_samples(T, stride)
    assert led.equity.shape == (P, market.shape[0], ns)
    assert led.equity_stride == stride
    at = np.minimum((np.arange(ns) + 1) * stride - 1, T - 1)
    np.testing.assert_array_equal(led.equity, full.equity[..., at])
    np.testing.assert_array_equal(led.equity[..., -1], full.metrics[..., 0])
    np.testing.assert_array_equal(full.equity[..., -1],
                                  full.metrics[..., 0])


def test_round_trips(run, market):
    fam, pop, _, led = run
    for p in range(P):
        for s in range(market.shape[0]):
            fills = led.fills(p, s)
            trips = led.round_trips(p, s)
            closed = [t for t in trips if t["reason"] != "open"]
            closing = [f for f in fills if f["kind"] in (
                "sell", "breakout", "take_profit")]
            assert len(closed) == led.metrics[p, s, 1]
            assert [t["pnl"] for t in closed] == [f["pnl"] for f in closing]
            assert [t["reason"] for t in closed] \
                == [f["kind"] for f in closing]
            assert all(t["exit_t"] >= t["entry_t"] >= 0 for t in closed)
            n_open = len(trips) - len(closed)
            if fam.name == "grid":
                # the fill mask at T, from the fills alone
                mask = 0
                for f in fills:
                    if f["kind"] in ("buy", "build"):
                        assert not mask >> f["slot"] & 1
                        mask |= 1 << f["slot"]
                    else:
                        assert mask >> f["slot"] & 1
                        mask &= ~(1 << f["slot"])
                assert n_open == bin(mask).count("1")
            else:
                in_cycle = bool(fills) and fills[-1]["kind"] != "take_profit"
                assert n_open == int(in_cycle)
    assert isinstance(led.numpy(), FillLedger) and led.numpy().t is led.t


# --- engine, analyzer, CLI on device="cpu" --------------------------------

GRID = {"half_levels": 6, "spacing_pct": 0.002}


@pytest.fixture(scope="module")
def engine_stats(tmp_path_factory):
    from ai_crypto_trader_amd.backtesting.engine import BacktestEngine
    d = tmp_path_factory.mktemp("fills_engine")
    eng = BacktestEngine(str(d), device="cpu")
    stats = eng.run_backtest("BTCUSDC", "grid", n_candles=3000, params=GRID,
                             record_fills=True, record_equity=True,
                             equity_stride=60)
    return d, eng, stats


def test_engine_stats(engine_stats):
    _, eng, stats = engine_stats
    assert stats["n_trades"] > 5
    assert stats["n_records"] == len(stats["fills"])
    assert {f["kind"] for f in stats["fills"]} <= set(FILL_KINDS[:4])
    assert len(stats["trades"]) == stats["n_trades"] + stats["n_open"]
    assert len(stats["equity_curve"]) == 3000 // 60
    assert stats["equity_curve"][-1] == stats["final_equity"]
    assert stats["equity_stride"] == 60
    for k in ("avg_win", "avg_loss", "max_win_streak", "max_loss_streak",
              "expectancy"):
        assert k in stats
    saved = json.loads(eng.last_saved.read_text())
    assert saved["fills"] == stats["fills"]
    assert saved["trades"] == stats["trades"]
    assert "equity_curve" not in saved
    # the same metrics as a plain run; capacity reaches the engine
    plain = eng.run_backtest("BTCUSDC", "grid", n_candles=3000, params=GRID)
    assert plain["final_equity"] == stats["final_equity"]
    assert "fills" not in plain
    with pytest.raises(ValueError, match="max_fills"):
        eng.run_backtest("BTCUSDC", "grid", n_candles=3000, params=GRID,
                         record_fills=True, max_fills=3)
    dca = eng.run_backtest("BTCUSDC", "dca", n_candles=3000,
                           record_fills=True)
    assert dca["fills"] and {f["kind"] for f in dca["fills"]} \
        <= set(FILL_KINDS[4:])


def test_engine_refuses_the_wrong_ledger(engine_stats):
    _, eng, _ = engine_stats
    with pytest.raises(ValueError, match="record_fills"):
        eng.run_backtest("BTCUSDC", "grid", n_candles=3000,
                         record_trades=True)
    with pytest.raises(ValueError, match="record_trades"):
        eng.run_backtest("BTCUSDC", "default", n_candles=3000,
                         record_fills=True)


def test_trade_analysis(engine_stats):
    from ai_crypto_trader_amd.backtesting.result_analyzer import (
        ResultAnalyzer,
    )
    d, _, stats = engine_stats
    ra = ResultAnalyzer(str(d / "analysis"))
    ta = ra.trade_analysis(stats)
    closed = [t for t in stats["trades"] if t["reason"] != "open"]
    assert set(ta["by_reason"]) <= {"sell", "breakout"}
    assert "sell" in ta["by_reason"]
    assert sum(r["count"] for r in ta["by_reason"].values()) \
        == len(closed) == stats["n_trades"]
    realized = sum(t["pnl"] for t in closed)
    assert sum(r["pnl"] for r in ta["by_reason"].values()) \
        == pytest.approx(realized, rel=1e-9)
    assert ta["n_open"] == stats["n_open"]
    assert ta["mean_duration"] > 0
    p = ra.plot_trade_analysis(stats)
    assert p.suffix == ".png" and p.stat().st_size > 1000


def test_cli_writes_the_csv_and_splits_by_regime(tmp_path):
    r = subprocess.run(
        [sys.executable, str(REPO / "run_backtest.py"), "--data-dir",
         str(tmp_path), "backtest", "--symbol", "BTCUSDC", "--cpu",
         "--strategy", "grid", "--candles", "3000", "--params",
         json.dumps(GRID), "--fills", "--equity-stride", "60", "--plot",
         "--by-regime"],
        capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "fill kind" in r.stdout and "build" in r.stdout
    assert "breakout" in r.stdout and "regime at entry" in r.stdout
    (saved,) = (tmp_path / "results").glob("*.json")
    (out,) = (tmp_path / "results").glob("*_fills.csv")
    assert out.name == saved.stem + "_fills.csv"
    with open(out) as f:
        rows = list(csv.DictReader(f))
    fills = json.loads(saved.read_text())["fills"]
    assert len(rows) == len(fills) > 0
    assert list(rows[0]) == list(FIELDS)
    assert rows[0]["kind"] == fills[0]["kind"] == "build"
    assert int(rows[-1]["t"]) == fills[-1]["t"]
    assert (tmp_path / "analysis" / "BTCUSDC_trades.png").exists()
    # --by-regime still needs a ledger to split
    r = subprocess.run(
        [sys.executable, str(REPO / "run_backtest.py"), "--data-dir",
         str(tmp_path), "backtest", "--symbol", "BTCUSDC", "--cpu",
         "--strategy", "grid", "--by-regime"],
        capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "--fills" in r.stderr
