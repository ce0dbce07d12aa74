"""Grid and DCA strategy families on the CPU: the numpy twins against
outcomes worked out by hand from the contracts in strategy_grid.py /
strategy_dca.py, the parameter helpers, and the family plumbing through
GAEngine, BacktestEngine and the CLI."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ai_crypto_trader_amd.backtesting import strategy_dca as sd
from ai_crypto_trader_amd.backtesting import strategy_grid as sg
from ai_crypto_trader_amd.backtesting.engine_dca_cpu import (
    rolling_max_close, run_dca_backtest_cpu,
)
from ai_crypto_trader_amd.backtesting.engine_grid_cpu import (
    run_grid_backtest_cpu,
)
from ai_crypto_trader_amd.backtesting.families import FAMILIES, get_family

REPO = Path(__file__).resolve().parent.parent
FEE = 0.001
OMF = 1.0 - FEE
# metric slots
EQ, NTR, WINS, GP, GL = 0, 1, 2, 3, 4


def series(rows):
    """[(close, high, low), ...] -> (1, T, 4) candles."""
    a = np.array([(c, h, lo, 1.0) for c, h, lo in rows], np.float32)
    return a[None]


# --- grid ---------------------------------------------------------------

# H=2, s=1 %, arithmetic, all equity committed, 5 % breakout band:
# levels 0.98 0.99 1.00 1.01 1.02 around close[0] = 1, b = 1/4.
GRID_H2 = np.array([[2, 0.01, 0, 1.0, 0.05]], np.float32)


def test_grid_one_rebuy_one_profitable_sell():
    # down one level (low 0.989 <= L[1] = 0.99) and back up (high 1.005
    # >= L[2] = 1.00); highs stay under L[3] = 1.01 so the two slots
    # bought at market never sell
    candles = series([(1.0, 1.0, 1.0),
                      (0.995, 1.0, 0.989),
                      (1.0, 1.005, 0.995)])
    m, curve = run_grid_backtest_cpu(candles, GRID_H2, record_equity=True)
    m = m[0, 0]
    b = 0.25
    u0 = b * OMF / 1.0
    u1 = b * OMF / 0.99                 # the rebuy at L[1]
    # t=0: two market slots -> cash 0.5; t=1: rebuy -> cash 0.25
    eq0 = 0.5 + 2 * u0 * 1.0
    eq1 = 0.25 + (2 * u0 + u1) * 0.995
    proceeds = u1 * 1.00 * OMF          # sold at L[2]
    eq2 = 0.25 + proceeds + 2 * u0 * 1.0
    assert m[NTR] == 1 and m[WINS] == 1
    assert proceeds - b > 0
    assert m[GP] == pytest.approx(proceeds - b, rel=1e-3)
    assert m[GL] == 0
    np.testing.assert_allclose(curve[0, 0], [eq0, eq1, eq2], rtol=1e-6)
    assert m[EQ] == pytest.approx(eq2, rel=1e-6)


def test_grid_no_buy_then_sell_within_one_candle():
    # one candle spans L[1] and L[2]: the rebuy at 0.99 must not sell at
    # 1.00 on the same candle — it sells on the next
    candles = series([(1.0, 1.0, 1.0),
                      (1.0, 1.005, 0.989),
                      (1.0, 1.005, 0.995)])
    m, curve = run_grid_backtest_cpu(candles, GRID_H2, record_equity=True)
    u0, u1 = 0.25 * OMF, 0.25 * OMF / 0.99
    assert curve[0, 0, 1] == pytest.approx(0.25 + (2 * u0 + u1), rel=1e-6)
    assert m[0, 0, NTR] == 1 and m[0, 0, WINS] == 1


def test_grid_breakout_liquidates_and_recentres():
    # gap down through both resting buys and past L[0]*(1-5%) = 0.931:
    # both buys fill (cash 0.5 -> 0), then all 4 filled slots are
    # liquidated at the close 0.90 (4 losing trades) and the grid is
    # rebuilt around 0.90: levels 0.882 0.891 0.900 0.909 0.918
    rows = [(1.0, 1.0, 1.0), (0.90, 1.0, 0.90)]
    m = run_grid_backtest_cpu(series(rows), GRID_H2)[0, 0]
    u0 = 0.25 * OMF
    units = 2 * u0 + 0.25 * OMF / 0.99 + 0.25 * OMF / 0.98
    cash = units * 0.90 * OMF
    b2 = cash / 4
    u0b = b2 * OMF / 0.90
    eq1 = (cash - 2 * b2) + 2 * u0b * 0.90
    assert m[NTR] == 4 and m[WINS] == 0
    assert m[EQ] == pytest.approx(eq1, rel=1e-6)
    # the rebuilt centre shows on the next candle: a high of 0.91 reaches
    # the NEW L[3] = 0.909 (one winning sell); around the old centre the
    # nearest sell level was 1.01 and nothing would trade
    rows.append((0.905, 0.91, 0.90))
    m = run_grid_backtest_cpu(series(rows), GRID_H2)[0, 0]
    assert m[NTR] == 5 and m[WINS] == 1
    proceeds = u0b * 0.909 * OMF
    eq2 = (cash - 2 * b2) + proceeds + u0b * 0.905
    assert m[EQ] == pytest.approx(eq2, rel=1e-6)


def test_grid_geometric_levels_and_cash_cap():
    # geometric: L[3] = 1*1.01, L[4] = L[3]*1.01 = 1.0201 — a high of
    # 1.0200 sells slot 2 only, 1.0201+ sells both market slots
    p = np.array([[2, 0.01, 1, 1.0, 0.05]], np.float32)
    m = run_grid_backtest_cpu(
        series([(1.0, 1.0, 1.0), (1.0, 1.02, 1.0)]), p)[0, 0]
    assert m[NTR] == 1
    m = run_grid_backtest_cpu(
        series([(1.0, 1.0, 1.0), (1.0, 1.0202, 1.0)]), p)[0, 0]
    assert m[NTR] == 2 and m[WINS] == 2


# --- DCA ----------------------------------------------------------------

def dca(period=4, base=0.01, dip=0.2, mult=2.0, cool=15, tp=0.2, va=0):
    return np.array([[period, base, dip, mult, cool, tp, va]], np.float32)


def test_dca_schedule_four_buys_in_sixteen_flat_candles():
    m, curve = run_dca_backtest_cpu(
        series([(1.0, 1.0, 1.0)] * 16), dca(), record_equity=True)
    # each buy of 0.01 costs its fee: equity steps down by 0.01*FEE at
    # t = 3, 7, 11, 15 and nowhere else
    steps = np.flatnonzero(np.diff(curve[0, 0], prepend=np.float32(1.0)))
    assert steps.tolist() == [3, 7, 11, 15]
    assert m[0, 0, NTR] == 0
    assert m[0, 0, EQ] == pytest.approx(1.0 - 4 * 0.01 * FEE, rel=1e-6)


def test_dca_take_profit_wins_and_resets_cycle():
    flat = (1.0, 1.0, 1.0)
    rows = [flat] * 4 + [(1.0, 1.02, 1.0)] + [flat] * 3
    # buy at t=3: units 0.00999, tp_price = 0.01/0.00999*1.01 = 1.01101;
    # t=4 high 1.02 sells there. Cycle restarts at t0=5: the next
    # scheduled buy is t=8, NOT t=7 (where n = 8 of the old cycle fell)
    units = 0.01 * OMF
    tp_price = 0.01 / units * 1.01
    pnl = units * tp_price * OMF - 0.01
    assert pnl > 0
    m = run_dca_backtest_cpu(series(rows), dca(tp=0.01))[0, 0]
    assert m[NTR] == 1 and m[WINS] == 1
    assert m[EQ] == pytest.approx(1.0 + pnl, rel=1e-6)
    m = run_dca_backtest_cpu(series(rows + [flat]), dca(tp=0.01))[0, 0]
    assert m[NTR] == 1
    assert m[EQ] == pytest.approx(1.0 + pnl - 0.01 * FEE, rel=1e-6)


def test_dca_dip_buy_respects_cooldown():
    rows = [(1.0, 1.0, 1.0)] * 5 + [(0.9, 0.9, 0.9)] * 16
    p = dca(period=720, dip=0.05, mult=2.0, cool=15)
    # 10 % under the rolling high at t=5 -> one dip buy of 2*base; the
    # dip persists but the cooldown blocks t=6..19; t=20 buys again
    m = run_dca_backtest_cpu(series(rows[:20]), p)[0, 0]
    assert m[EQ] == pytest.approx(1.0 - 0.02 * FEE, rel=1e-7)
    m = run_dca_backtest_cpu(series(rows), p)[0, 0]
    assert m[EQ] == pytest.approx(1.0 - 2 * 0.02 * FEE, rel=1e-7)


def test_dca_value_averaging_buys_the_gap():
    rows = [(1.0, 1.0, 1.0)] * 8 + [(0.9, 0.9, 0.9)] * 4
    # targets 0.01, 0.02, 0.03 at t = 3, 7, 11
    u = 0.01 * OMF                              # t=3: gap 0.01
    usd2 = 0.02 - u * 1.0                       # t=7
    u += usd2 * OMF
    usd3 = 0.03 - u * 0.9                       # t=11, after the drop
    assert 0.01 < usd3 < 0.04
    u_end = u + usd3 * OMF / 0.9
    cash = 1.0 - 0.01 - usd2 - usd3
    m = run_dca_backtest_cpu(series(rows), dca(va=1))[0, 0]
    assert m[EQ] == pytest.approx(cash + u_end * 0.9, rel=1e-6)
    fixed = run_dca_backtest_cpu(series(rows), dca(va=0))[0, 0]
    assert fixed[EQ] != m[EQ]


def test_rolling_max_close_window():
    close = np.concatenate([[5.0], np.ones(130)]).astype(np.float32)
    c = np.zeros((1, close.size, 4), np.float32)
    c[0, :, 0] = close
    r = rolling_max_close(c)[0]
    assert r[0] == 5 and r[119] == 5 and r[120] == 1   # 120-candle window


# --- parameter helpers --------------------------------------------------

@pytest.mark.parametrize("name", ["grid", "dca"])
def test_clip_and_random_population_respect_bounds(name):
    fam = get_family(name)
    lo, hi, is_int = fam.bounds.T
    pop = fam.random_population(200, seed=3)
    assert pop.shape == (200, fam.nparam) and pop.dtype == np.float32
    assert (pop >= lo).all() and (pop <= hi).all()
    ints = pop[:, is_int > 0]
    assert (ints == np.rint(ints)).all()
    np.testing.assert_array_equal(pop, fam.random_population(200, seed=3))
    wild = np.random.default_rng(0).normal(0, 1000, (50, fam.nparam))
    c = fam.clip(wild.astype(np.float32))
    assert (c >= lo).all() and (c <= hi).all()
    assert (c[:, is_int > 0] == np.rint(c[:, is_int > 0])).all()
    d = fam.params_to_dict(pop[0])
    assert list(d) == fam.names
    np.testing.assert_array_equal(fam.dict_to_params(d), pop[0])
    assert len(fam.names) == fam.nparam == fam.bounds.shape[0]
    assert fam.bounds.shape[1] == 3


def test_from_config_mapping():
    from ai_crypto_trader_amd.config import DCAConfig, GridConfig

    g = sg.from_config(GridConfig(levels=10, spacing="geometric",
                                  range_pct=0.05))
    d = sg.grid_params_to_dict(g)
    assert d["half_levels"] == 5 and d["geometric"] == 1
    assert d["spacing_pct"] == pytest.approx(0.01)
    assert sg.from_config(GridConfig())[2] == 0
    v = sd.from_config(DCAConfig(schedule="value_averaging",
                                 dip_threshold_pct=0.07,
                                 dip_multiplier=3.0))
    d = sd.dca_params_to_dict(v)
    assert d["value_averaging"] == 1
    assert d["dip_threshold_pct"] == pytest.approx(0.07)
    assert d["dip_multiplier"] == pytest.approx(3.0)
    assert sd.from_config(DCAConfig())[6] == 0


# --- plumbing -----------------------------------------------------------

@pytest.fixture(scope="module")
def volatile_market():
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(1200, 2, seed=7, sigma=3.0))


@pytest.mark.parametrize("name", ["grid", "dca"])
def test_ga_engine_family_cpu(name, volatile_market):
    from ai_crypto_trader_amd.backtesting.ga_engine import GAEngine

    fam = FAMILIES[name]
    lo, hi, is_int = fam.bounds.T

    def run():
        eng = GAEngine(volatile_market, pop_per_rank=24, device="cpu",
                       seed=5, family=name)
        for _ in range(2):
            eng.step()
            assert np.isfinite(eng.last_fitness_global.numpy()).all()
        return eng.pop_t.numpy()

    pop = run()
    assert pop.shape == (24, fam.nparam)
    assert (pop >= lo).all() and (pop <= hi).all()
    assert (pop[:, is_int > 0] == np.rint(pop[:, is_int > 0])).all()
    np.testing.assert_array_equal(pop, run())


def test_ga_engine_family_rejects_continuous(volatile_market):
    from ai_crypto_trader_amd.backtesting.ga_engine import GAEngine

    with pytest.raises(AssertionError):
        GAEngine(volatile_market, pop_per_rank=8, device="cpu",
                 family="grid", continuous=True)
    with pytest.raises(ValueError):
        GAEngine(volatile_market, pop_per_rank=8, device="cpu",
                 family="martingale")


@pytest.mark.parametrize("name", ["grid", "dca"])
def test_backtest_engine_routes_family(name, tmp_path):
    from ai_crypto_trader_amd.backtesting.engine import BacktestEngine

    eng = BacktestEngine(str(tmp_path / "d"), device="cpu")
    stats = eng.run_backtest("BTCUSDC", name, n_candles=1500,
                             record_equity=True)
    for k in ("final_equity", "total_return_pct", "win_rate",
              "profit_factor", "sharpe", "max_drawdown_pct", "n_trades",
              "fitness", "candles_per_sec"):
        assert k in stats
    assert stats["strategy"] == name and stats["engine"] == "cpu"
    assert list(stats["params"]) == FAMILIES[name].names
    assert len(stats["equity_curve"]) == 1500
    assert stats["equity_curve"][-1] == pytest.approx(
        stats["final_equity"])
    # params dicts use the family's names
    key = FAMILIES[name].names[1]
    val = float(FAMILIES[name].bounds[1, 1])
    s2 = eng.run_backtest("BTCUSDC", name, n_candles=1500,
                          params={key: val})
    assert s2["params"][key] == pytest.approx(val)


def test_cli_optimize_grid_cpu(tmp_path):
    d = str(tmp_path / "cli")
    cli = [sys.executable, str(REPO / "run_backtest.py"), "--data-dir", d]
    r = subprocess.run(
        cli + ["fetch", "--symbol", "SOLUSDC", "--candles", "1200"],
        capture_output=True, text=True, timeout=180, cwd=REPO)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(
        cli + ["optimize", "--symbol", "SOLUSDC", "--strategy", "grid",
               "--pop", "16", "--generations", "2", "--candles", "1200",
               "--cpu"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["strategy"] == "grid"
    assert list(out["params"]) == sg.GRID_PARAM_NAMES
    assert len(out["optimize"]["fitness_history"]) == 2
    assert np.isfinite(out["optimize"]["best_fitness"])
