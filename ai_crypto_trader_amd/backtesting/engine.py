"""Backtest orchestrator (reference parity: backtesting/backtest_engine.py
:14-325 + strategy_tester.py:17-487).

run_backtest() fetches-if-missing then runs the per-candle engine —
the CPU reference engine for small runs and the HIP backtest kernel on
GPU (one lane per param-set x symbol) — and produces the final-stats dict
(strategy_tester.py:403-430 formulas: total return, win rate, profit
factor, annualized Sharpe, max drawdown). Multi-symbol x param sweeps and
GA-based parameter optimization ride the same kernels (SURVEY.md §3.2:
the reference's per-candle OpenAI call is replaced by deterministic
parameterized strategies, which is what makes the loop a pure kernel)."""

from __future__ import annotations

import json
import time
from pathlib import Path

import numpy as np

from ..backtesting.engine_cpu import (
    METRIC_NAMES, run_backtest_cpu,
)
from ..backtesting.strategy import (
    clip_params, dict_to_params, params_to_dict,
)
from ..ops import gpu_available
from .families import FAMILIES
from .fills import DEFAULT_MAX_FILLS
from .ledger import DEFAULT_MAX_TRADES
from .data_manager import HistoricalDataManager

ANNUAL_CANDLES = 525_600.0      # 1m bars

# bars per year by interval (interval-aware Sharpe annualization)
INTERVAL_BARS_PER_YEAR = {
    "1m": 525_600.0, "3m": 175_200.0, "5m": 105_120.0,
    "15m": 35_040.0, "30m": 17_520.0, "1h": 8_760.0,
    "4h": 2_190.0, "1d": 365.0,
}


# Named strategy presets of the vote state machine. "dca_strategy" is such
# a preset (DCA-like cadence and sizing through votes) and is kept for
# compatibility; the real resting-order grid and scheduled/dip-buy DCA
# semantics of the reference's bots (grid_trading_strategy.py,
# dca_strategy.py:347-741) live in the strategy families "grid" and "dca"
# (backtesting/families.py), which run_backtest() routes to by name.
STRATEGY_PRESETS = {
    "default": {},
    "dca_strategy": {
        "entry_votes": 1, "exit_votes": 3, "position_size_pct": 0.1,
        "stop_loss_pct": 0.2, "take_profit_pct": 0.4,
        "trailing_stop_pct": 0.0,
    },
    "momentum": {
        "entry_votes": 2, "exit_votes": 2, "position_size_pct": 0.5,
        "stop_loss_pct": 0.02, "take_profit_pct": 0.05,
        "trailing_stop_pct": 0.01, "trailing_act_pct": 0.02,
    },
    "mean_reversion": {
        "rsi_oversold": 25.0, "rsi_overbought": 75.0, "bb_buy_th": 0.02,
        "bb_sell_th": 0.98, "entry_votes": 2, "exit_votes": 1,
        "take_profit_pct": 0.02, "stop_loss_pct": 0.03,
    },
    "conservative": {
        "entry_votes": 3, "exit_votes": 1, "position_size_pct": 0.2,
        "stop_loss_pct": 0.01, "take_profit_pct": 0.03,
    },
}


def metrics_to_stats(m: np.ndarray, T: int, interval: str = "1m") -> dict:
    """One lane's metric vector -> result dict
    (strategy_tester.py:403-430 / strategy_evaluation.py:32-228).
    Sharpe is recomputed HOST-SIDE from the kernel's raw return moments
    (sum_ret/sum_ret2) with the interval's bars-per-year, so non-1m
    backtests annualize correctly (the in-kernel sharpe/fitness are
    1m-annualized — the GA fitness convention)."""
    d = dict(zip(METRIC_NAMES, (float(x) for x in m)))
    gp, gl = d["gross_profit"], d["gross_loss"]
    bars_py = INTERVAL_BARS_PER_YEAR.get(interval, ANNUAL_CANDLES)
    years = T / bars_py
    n = max(T, 1)
    mean_r = d["sum_ret"] / n
    var_r = max(d["sum_ret2"] / n - mean_r * mean_r, 0.0)
    sharpe = (mean_r / max(np.sqrt(var_r), 1e-9) * np.sqrt(bars_py)
              if d["n_trades"] > 0 else 0.0)
    d["sharpe"] = float(sharpe)
    return {
        "final_equity": d["final_equity"],
        "total_return_pct": (d["final_equity"] - 1.0) * 100.0,
        "annualized_return_pct":
            ((d["final_equity"] ** (1 / max(years, 1e-9))) - 1.0) * 100.0
            if d["final_equity"] > 0 else -100.0,
        "n_trades": int(d["n_trades"]),
        "win_rate": d["wins"] / max(d["n_trades"], 1.0),
        # capped: float('inf') serializes as the non-standard 'Infinity'
        # token that strict JSON parsers (and dashboards) reject
        "profit_factor": min(gp / gl, 1e9) if gl > 0 else (
            1e9 if gp > 0 else 0.0),
        "max_drawdown_pct": d["max_drawdown"] * 100.0,
        "sharpe": d["sharpe"],
        "fitness": d["fitness"],
    }


class BacktestEngine:
    def __init__(self, data_dir: str = "backtesting_data",
                 device: str | None = None):
        self.dm = HistoricalDataManager(data_dir)
        if device is None:
            device = "cuda" if gpu_available() else "cpu"
        self.device = device
        self.results_dir = Path(data_dir) / "results"
        self.results_dir.mkdir(parents=True, exist_ok=True)
        self.last_saved: Path | None = None      # newest results JSON
        self.last_candles: np.ndarray | None = None   # of the newest run

    # --- single run ------------------------------------------------------
    def run_backtest(self, symbol: str, strategy: str = "default",
                     interval: str = "1m", n_candles: int = 10_000,
                     params: dict | None = None,
                     record_equity: bool = False,
                     record_trades: bool = False,
                     max_trades: int = DEFAULT_MAX_TRADES,
                     equity_stride: int = 1,
                     record_fills: bool = False,
                     max_fills: int = DEFAULT_MAX_FILLS) -> dict:
        """record_trades (vote machine only) adds the trade ledger to the
        stats: `trades` (backtesting/ledger.py records as dicts, at most
        max_trades), `n_open`, and the trade-derived numbers of
        evaluation.calculate_metrics / calculate_advanced_metrics.
        equity_stride thins the recorded equity curve (vote machine, and a
        family run with record_fills).

        record_fills (grid / dca families only) adds the fill ledger:
        `fills` (backtesting/fills.py records as dicts, at most
        max_fills), `n_records`, `trades` (the fills folded into round
        trips, FillLedger.round_trips — it needs every fill, so a lane
        that overflows max_fills raises ValueError), `n_open` and the same
        trade-derived numbers."""
        df = self.dm.load_market_data(symbol, interval,
                                      n_candles=n_candles)
        candles = self.dm.to_chlv(df.iloc[:n_candles])
        self.last_candles = candles     # (1, T, 4), for per-candle labels
        fam = FAMILIES.get(strategy)
        if fam is not None:
            vec = fam.clip(fam.dict_to_params(params or {})[None])
            to_dict = fam.params_to_dict
        else:
            preset = dict(STRATEGY_PRESETS.get(strategy, {}))
            if params:
                preset.update(params)
            vec = clip_params(dict_to_params(preset)[None])
            to_dict = params_to_dict
        if fam is not None and record_trades:
            raise ValueError(
                f"no trade ledger for the {strategy!r} family: its fills "
                "are per level / per order, not one position at a time; "
                "record_fills=True records them")
        if fam is None and record_fills:
            raise ValueError(
                f"no fill ledger for the vote machine ({strategy!r}): it "
                "holds one position at a time; record_trades=True records "
                "its trades")
        ledger = None
        t0 = time.perf_counter()
        if record_fills:
            ledger = self._run_fills(fam, candles, vec, max_fills,
                                     equity_stride)
            metrics = ledger.metrics
        elif fam is None and (record_trades or record_equity):
            ledger = self._run_ledger(candles, vec, max_trades,
                                      equity_stride)
            metrics = ledger.metrics
        else:
            out = self._run(candles, vec, record_equity, fam)
            metrics = out[0] if record_equity else out
        elapsed = time.perf_counter() - t0
        T = candles.shape[1]
        stats = metrics_to_stats(metrics[0, 0], T, interval)
        stats.update({
            "symbol": symbol, "strategy": strategy, "interval": interval,
            "n_candles": T, "engine": self.device,
            "candles_per_sec": T / max(elapsed, 1e-9),
            "params": to_dict(vec[0]),
        })
        if ledger is not None:
            if record_equity:
                stats["equity_curve"] = ledger.equity[0, 0].tolist()
                stats["equity_stride"] = ledger.equity_stride
            if record_trades:
                stats.update(self._trade_stats(ledger))
            if record_fills:
                stats["fills"] = ledger.fills(0, 0)
                stats.update(self._trade_stats(
                    ledger, ledger.round_trips(0, 0)))
        elif record_equity:
            stats["equity_curve"] = out[1][0, 0].tolist()
        self._save(stats)
        return stats

    def _run_ledger(self, candles: np.ndarray, pop: np.ndarray,
                    max_trades: int, equity_stride: int):
        """Vote machine with the trade ledger: the HIP ledger kernel on a
        GPU, its numpy twin on CPU — the same `Ledger`, as numpy."""
        if self.device.startswith("cuda"):
            import torch

            from ..ops.backtest import run_backtest_ledger_gpu
            led = run_backtest_ledger_gpu(
                torch.from_numpy(candles).to(self.device),
                torch.from_numpy(pop).to(self.device),
                max_trades=max_trades, equity_stride=equity_stride)
            torch.cuda.synchronize()
            return led.numpy()
        return run_backtest_cpu(candles, pop, record_trades=True,
                                max_trades=max_trades,
                                equity_stride=equity_stride)

    def _run_fills(self, fam, candles: np.ndarray, pop: np.ndarray,
                   max_fills: int, equity_stride: int):
        """A family with the fill ledger: the HIP fills kernel on a GPU,
        the numpy twin on CPU — the same `FillLedger`, as numpy."""
        if self.device.startswith("cuda"):
            import torch

            led = fam.run_gpu_fills(
                torch.from_numpy(candles).to(self.device),
                torch.from_numpy(pop).to(self.device),
                max_fills=max_fills, equity_stride=equity_stride)
            torch.cuda.synchronize()
            return led.numpy()
        return fam.run_cpu_fills(candles, pop, max_fills=max_fills,
                                 equity_stride=equity_stride)

    @staticmethod
    def _trade_stats(ledger, trades: list | None = None) -> dict:
        """Lane (0, 0)'s records (a fill ledger's: its round trips, passed
        in) and what only a trade list can say: avg win/loss, streaks,
        per-trade expectancy."""
        from .evaluation import (
            calculate_advanced_metrics, calculate_metrics,
        )
        if trades is None:
            trades = ledger.trades(0, 0)
        closed = [t for t in trades if t["reason"] != "open"]
        out = {
            "trades": trades,
            "n_open": len(trades) - len(closed),
            "n_records": int(ledger.n_records[0, 0]),
            "avg_win": 0.0, "avg_loss": 0.0, "max_win_streak": 0,
            "max_loss_streak": 0, "expectancy": 0.0,
        }
        if closed:
            eq = ledger.equity[0, 0]
            basic = calculate_metrics(eq, closed)
            adv = calculate_advanced_metrics(eq, closed)
            out.update({k: basic[k] for k in ("avg_win", "avg_loss")})
            out.update({k: adv[k] for k in (
                "max_win_streak", "max_loss_streak", "expectancy")})
        return out

    def _run(self, candles: np.ndarray, pop: np.ndarray,
             record_equity: bool = False, fam=None):
        if self.device.startswith("cuda") and not record_equity:
            import torch

            from ..ops.backtest import run_backtest_gpu
            c = torch.from_numpy(candles).to(self.device)
            p = torch.from_numpy(pop).to(self.device)
            m = (fam.run_gpu if fam is not None else run_backtest_gpu)(c, p)
            torch.cuda.synchronize()
            return m.cpu().numpy()
        run_cpu = fam.run_cpu if fam is not None else run_backtest_cpu
        return run_cpu(candles, pop, record_equity=record_equity)

    # --- sweeps (reference :127-178) -------------------------------------
    def run_multiple_backtests(self, symbols: list[str],
                               strategies: list[str],
                               n_candles: int = 10_000) -> dict:
        results = []
        for sym in symbols:
            for strat in strategies:
                results.append(self.run_backtest(sym, strat,
                                                 n_candles=n_candles))
        best = max(results, key=lambda r: r["sharpe"])
        return {
            "results": results,
            "best": {"symbol": best["symbol"], "strategy": best["strategy"],
                     "sharpe": best["sharpe"]},
        }

    # --- one strategy, a basket of symbols, one account -------------------
    def run_portfolio_backtest(self, symbols: list[str], *,
                               max_positions: int,
                               strategy: str = "default",
                               params: dict | None = None,
                               use_gpu: bool | None = None,
                               equity_stride: int = 1,
                               interval: str = "1m",
                               n_candles: int = 10_000) -> dict:
        """One vote-machine strategy trading all `symbols` from one cash
        account with at most `max_positions` open at once (the portfolio
        position machine, backtesting/portfolio.py) — where
        run_multiple_backtests gives every symbol the whole account.

        The symbols' histories are cut to their common length and each is
        normalised to its first close, as run_backtest does. use_gpu None
        follows the engine's device. The stats are metrics_to_stats of the
        portfolio plus `per_symbol` (trades, win rate and realised pnl of
        each symbol's own exits), `refused_slots` / `refused_cash` (entry
        signals left untaken because every slot was taken / no cash was
        left) and, with equity_stride > 0, the sampled `equity_curve`."""
        from .portfolio import check_shape

        symbols = list(symbols)
        if strategy in FAMILIES:
            raise ValueError(
                f"the portfolio machine trades the vote machine's signals; "
                f"the {strategy!r} family has no portfolio form")
        check_shape(len(symbols), int(max_positions), int(equity_stride))
        if len(set(symbols)) != len(symbols):
            raise ValueError(f"a symbol is listed twice: {symbols}")
        frames = [self.dm.load_market_data(s, interval, n_candles=n_candles)
                  for s in symbols]
        T = min(n_candles, *(len(df) for df in frames))
        candles = np.concatenate(
            [self.dm.to_chlv(df.iloc[:T]) for df in frames], axis=0)
        self.last_candles = candles
        preset = dict(STRATEGY_PRESETS.get(strategy, {}))
        if params:
            preset.update(params)
        vec = clip_params(dict_to_params(preset)[None])
        on_gpu = (self.device.startswith("cuda") if use_gpu is None
                  else bool(use_gpu))
        t0 = time.perf_counter()
        if on_gpu:
            import torch

            from ..ops.backtest import run_backtest_portfolio_gpu
            dev = self.device if self.device.startswith("cuda") else "cuda"
            res = run_backtest_portfolio_gpu(
                torch.from_numpy(candles).to(dev),
                torch.from_numpy(vec).to(dev), max_positions=max_positions,
                equity_stride=equity_stride)
            torch.cuda.synchronize()
            res = res.numpy()
        else:
            from .engine_portfolio_cpu import run_portfolio_backtest_cpu
            res = run_portfolio_backtest_cpu(
                candles, vec, max_positions=max_positions,
                equity_stride=equity_stride)
        elapsed = time.perf_counter() - t0
        stats = metrics_to_stats(res.metrics[0], T, interval)
        head = "_".join(symbols[:3])
        more = f"_and{len(symbols) - 3}" if len(symbols) > 3 else ""
        stats.update({
            "symbol": f"PORTFOLIO_{head}{more}", "symbols": symbols,
            "strategy": strategy, "interval": interval, "n_candles": T,
            "max_positions": int(max_positions),
            "engine": "cuda" if on_gpu else "cpu",
            "candles_per_sec": len(symbols) * T / max(elapsed, 1e-9),
            "params": params_to_dict(vec[0]),
            "refused_slots": int(res.refused[0, 0]),
            "refused_cash": int(res.refused[0, 1]),
            "per_symbol": [
                {"symbol": s, "n_trades": int(n), "wins": int(w),
                 "win_rate": float(w) / max(float(n), 1.0),
                 "gross_profit": float(gp), "gross_loss": float(gl),
                 "pnl": float(gp) - float(gl)}
                for s, (n, w, gp, gl) in zip(symbols, res.per_symbol[0])],
        })
        if res.equity is not None:
            stats["equity_curve"] = res.equity[0].tolist()
            stats["equity_stride"] = res.equity_stride
        self._save(stats)
        return stats

    # --- GA parameter optimization over the GPU kernel -------------------
    def optimize(self, symbol: str, pop_size: int = 256,
                 generations: int = 10, n_candles: int = 20_000,
                 seed: int = 0, strategy: str = "vote",
                 record_trades: bool = False,
                 record_fills: bool = False,
                 max_fills: int = DEFAULT_MAX_FILLS) -> dict:
        """strategy: "vote" (the vote machine) or a family name ("grid",
        "dca") — the GA then searches that family's parameter space.
        record_trades: the final run of the winner keeps its trade ledger
        (vote machine only). record_fills: it keeps its fill ledger (a
        family only)."""
        from .ga_engine import GAEngine

        df = self.dm.load_market_data(symbol, n_candles=n_candles)
        candles = self.dm.to_chlv(df.iloc[:n_candles])
        eng = GAEngine(candles, pop_per_rank=pop_size, device=self.device,
                       seed=seed, segments="auto", family=strategy)
        fam = FAMILIES.get(strategy)
        t0 = time.perf_counter()
        history = []
        for _ in range(generations):
            eng.step()
            history.append(float(eng.last_fitness_global.max()))
        eng.eval_fitness()
        elapsed = time.perf_counter() - t0
        fit, best = eng.best()
        if fam is not None:
            stats = self.run_backtest(symbol, strategy,
                                      params=fam.params_to_dict(best),
                                      n_candles=n_candles,
                                      record_fills=record_fills,
                                      max_fills=max_fills)
        else:
            stats = self.run_backtest(symbol, "optimized",
                                      params=params_to_dict(best),
                                      n_candles=n_candles,
                                      record_trades=record_trades)
        stats["optimize"] = {
            "pop_size": pop_size, "generations": generations,
            "best_fitness": fit, "fitness_history": history,
            "candle_evals_per_sec":
                eng.candle_evals_per_step * generations / elapsed,
        }
        return stats

    def _save(self, stats: dict):
        name = (f"{stats['symbol']}_{stats['strategy']}_"
                f"{int(time.time())}.json")
        slim = {k: v for k, v in stats.items() if k != "equity_curve"}
        self.last_saved = self.results_dir / name
        with open(self.last_saved, "w") as f:
            json.dump(slim, f, indent=2)

    def list_results(self) -> list[dict]:
        out = []
        for p in sorted(self.results_dir.glob("*.json")):
            with open(p) as f:
                out.append(json.load(f))
        return out
