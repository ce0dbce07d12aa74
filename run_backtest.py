#!/usr/bin/env python3
"""Backtesting CLI (reference parity: run_backtest.py:24-227 — subcommands
fetch / backtest / list / analyze, plus `optimize` for GA parameter search
over the GPU backtest kernel).

Examples:
  python run_backtest.py fetch --symbol BTCUSDC --candles 20000
  python run_backtest.py backtest --symbol BTCUSDC --strategy dca_strategy
  python run_backtest.py backtest --symbol BTCUSDC --strategy momentum --plot
  python run_backtest.py backtest --symbol BTCUSDC --trades --equity-stride 60
  python run_backtest.py optimize --symbol BTCUSDC --pop 256 --generations 10
  python run_backtest.py optimize --symbol BTCUSDC --strategy grid
  python run_backtest.py backtest --symbol BTCUSDC --strategy dca
  python run_backtest.py backtest --symbol BTCUSDC --strategy grid --fills \
      --by-regime --plot
  python run_backtest.py backtest --portfolio BTCUSDC,ETHUSDC,SOLUSDC \
      --max-positions 2 --plot
  python run_backtest.py list
  python run_backtest.py analyze [--metric sharpe_ratio]
"""

from __future__ import annotations

import argparse
import csv
import json

from ai_crypto_trader_amd.backtesting.data_manager import (
    HistoricalDataManager,
)
from ai_crypto_trader_amd.backtesting.engine import (
    STRATEGY_PRESETS, BacktestEngine,
)
from ai_crypto_trader_amd.backtesting.families import FAMILIES
from ai_crypto_trader_amd.backtesting.fills import (
    DEFAULT_MAX_FILLS, FIELDS as FILL_FIELDS, FILL_KINDS,
)
from ai_crypto_trader_amd.backtesting.ledger import (
    DEFAULT_MAX_TRADES, FIELDS, REASONS,
)
from ai_crypto_trader_amd.backtesting.result_analyzer import ResultAnalyzer


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--data-dir", default="backtesting_data")
    sub = ap.add_subparsers(dest="cmd", required=True)

    f = sub.add_parser("fetch", help="fetch (synthesize) historical data")
    f.add_argument("--symbol", required=True)
    f.add_argument("--interval", default="1m")
    f.add_argument("--candles", type=int, default=10_000)
    f.add_argument("--social", action="store_true")

    b = sub.add_parser("backtest", help="run a backtest")
    b.add_argument("--symbol", default=None,
                   help="required unless --portfolio is given")
    b.add_argument("--portfolio", type=str, default=None,
                   metavar="SYM1,SYM2,...",
                   help="trade this basket of symbols (at most 64) with one "
                        "vote-machine strategy from ONE cash account: "
                        "prints the portfolio stats, the per-symbol table "
                        "and how many entry signals went untaken")
    b.add_argument("--max-positions", type=int, default=None,
                   help="with --portfolio: positions open at once "
                        "(default: all symbols)")
    b.add_argument("--strategy", default="default",
                   choices=sorted([*STRATEGY_PRESETS, *FAMILIES]),
                   help="a vote-machine preset, or the strategy family "
                        "grid / dca")
    b.add_argument("--interval", default="1m")
    b.add_argument("--candles", type=int, default=10_000)
    b.add_argument("--cpu", action="store_true",
                   help="force the CPU reference engine")
    b.add_argument("--plot", action="store_true")
    b.add_argument("--params", type=str, default=None,
                   help="JSON dict of parameter overrides")
    b.add_argument("--trades", action="store_true",
                   help="record the trade ledger (vote machine): print "
                        "the per-exit-reason table and write a "
                        "*_trades.csv next to the saved JSON")
    b.add_argument("--fills", action="store_true",
                   help="record the fill ledger (grid / dca family): print "
                        "the per-kind and per-exit-reason tables and write "
                        "a *_fills.csv next to the saved JSON")
    b.add_argument("--by-regime", action="store_true",
                   help="with --trades or --fills: label the history with "
                        "the regime detector (HMM) and print the closed "
                        "trades (round trips) split by the regime at entry")
    b.add_argument("--max-trades", type=int, default=DEFAULT_MAX_TRADES,
                   help="trade records kept (the newest are dropped)")
    b.add_argument("--max-fills", type=int, default=DEFAULT_MAX_FILLS,
                   help="fill records kept (the newest are dropped)")
    b.add_argument("--equity-stride", type=int, default=1,
                   help="keep every Nth candle of the equity curve")

    o = sub.add_parser("optimize", help="GA parameter search")
    o.add_argument("--symbol", required=True)
    o.add_argument("--pop", type=int, default=256)
    o.add_argument("--generations", type=int, default=10)
    o.add_argument("--candles", type=int, default=20_000)
    o.add_argument("--cpu", action="store_true")
    o.add_argument("--strategy", default="vote",
                   choices=["vote", *sorted(FAMILIES)],
                   help="parameter space to search: the vote machine or "
                        "the grid / dca strategy family")

    sub.add_parser("list", help="list stored data and results")
    an = sub.add_parser("analyze",
                        help="summary report over stored results")
    an.add_argument("--metric", default=None,
                    help="rank results by this metric only (reference "
                         "run_backtest.py `analyze --metric "
                         "sharpe_ratio`); aliases: sharpe_ratio, "
                         "total_return, win_rate, profit_factor")

    args = ap.parse_args()
    if (getattr(args, "by_regime", False)
            and not (args.trades or args.fills)):
        ap.error("--by-regime splits the trade ledger: it needs --trades "
                 "(vote machine) or --fills (grid / dca)")
    if args.cmd == "backtest":
        if args.portfolio is None and args.symbol is None:
            ap.error("backtest needs --symbol (or --portfolio SYM1,SYM2,...)")
        if args.portfolio is not None and (
                args.symbol or args.trades or args.fills):
            ap.error("--portfolio takes the place of --symbol and keeps no "
                     "per-trade ledger (--trades / --fills)")
        if args.portfolio is None and args.max_positions is not None:
            ap.error("--max-positions goes with --portfolio")
    dm = HistoricalDataManager(args.data_dir)

    if args.cmd == "fetch":
        df = dm.fetch_market_data(args.symbol, args.interval, args.candles)
        print(f"fetched {len(df)} {args.interval} candles for "
              f"{args.symbol} -> {dm.market_path(args.symbol, args.interval)}")
        if args.social:
            sdf = dm.fetch_social_data(args.symbol)
            print(f"fetched {len(sdf)} social rows -> "
                  f"{dm.social_path(args.symbol)}")
        return

    if args.cmd == "backtest":
        eng = BacktestEngine(args.data_dir,
                             device="cpu" if args.cpu else None)
        params = json.loads(args.params) if args.params else None
        if args.portfolio is not None:
            symbols = [x for x in args.portfolio.split(",") if x]
            try:
                stats = eng.run_portfolio_backtest(
                    symbols,
                    max_positions=(len(symbols) if args.max_positions is None
                                   else args.max_positions),
                    strategy=args.strategy, params=params,
                    equity_stride=args.equity_stride if args.plot else 0,
                    interval=args.interval, n_candles=args.candles)
            except ValueError as e:
                raise SystemExit(f"--portfolio: {e}")
            if args.plot:
                ra = ResultAnalyzer(f"{args.data_dir}/analysis")
                print(f"plot -> {ra.plot_equity_curve(stats)}")
                stats.pop("equity_curve", None)
            rows = stats.pop("per_symbol")
            print(json.dumps(stats, indent=2, default=str))
            stats["per_symbol"] = rows
            print(f"{'symbol':<14} {'trades':>6} {'win rate':>9} "
                  f"{'pnl':>12}")
            for r in rows:
                print(f"{r['symbol']:<14} {r['n_trades']:>6} "
                      f"{r['win_rate']:>9.3f} {r['pnl']:>12.6f}")
            print(f"{'portfolio':<14} {stats['n_trades']:>6} "
                  f"{stats['win_rate']:>9.3f} "
                  f"{sum(r['pnl'] for r in rows):>12.6f}   entry signals "
                  f"untaken: {stats['refused_slots']} for slots, "
                  f"{stats['refused_cash']} for cash")
            return
        stats = eng.run_backtest(
            args.symbol, args.strategy, args.interval, args.candles,
            params=params, record_equity=args.plot,
            record_trades=args.trades, max_trades=args.max_trades,
            equity_stride=args.equity_stride, record_fills=args.fills,
            max_fills=args.max_fills)
        ra = ResultAnalyzer(f"{args.data_dir}/analysis")
        if args.plot:
            p = ra.plot_equity_curve(stats)
            print(f"plot -> {p}")
            stats.pop("equity_curve", None)
            if stats.get("trades"):
                print(f"trade plot -> {ra.plot_trade_analysis(stats)}")
        trades = stats.pop("trades", None)
        fills = stats.pop("fills", None)
        print(json.dumps(stats, indent=2, default=str))
        if fills is not None:
            stats["fills"] = fills
            print(f"{'fill kind':<14} {'count':>6} {'units':>14} "
                  f"{'cash':>14}")
            for kind in FILL_KINDS:
                rows = [f for f in fills if f["kind"] == kind]
                if rows:
                    print(f"{kind:<14} {len(rows):>6} "
                          f"{sum(f['units'] for f in rows):>14.6f} "
                          f"{sum(f['cash'] for f in rows):>14.6f}")
            path = eng.last_saved.with_name(
                eng.last_saved.stem + "_fills.csv")
            with open(path, "w", newline="") as f:
                w = csv.DictWriter(f, fieldnames=list(FILL_FIELDS))
                w.writeheader()
                w.writerows(fills)
            print(f"fills -> {path}")
        if trades is not None:
            stats["trades"] = trades
            if args.by_regime:
                from ai_crypto_trader_amd.backtesting.evaluation import (
                    label_regimes,
                )
                from ai_crypto_trader_amd.services.market_regime import (
                    REGIMES,
                )
                try:
                    labels = label_regimes(
                        eng.last_candles,
                        device=eng.device if eng.device.startswith("cuda")
                        else None)[0]
                except ValueError as e:
                    raise SystemExit(f"--by-regime: {e}")
                stats["regime_at_entry"] = [
                    REGIMES[labels[t["entry_t"]]]
                    if labels[t["entry_t"]] >= 0 else "unlabelled"
                    for t in trades]
            ta = ra.trade_analysis(stats)
            print(f"{'exit reason':<14} {'count':>6} {'pnl':>12}")
            for r in (REASONS[1:] if fills is None
                      else ("sell", "breakout", "take_profit")):
                row = ta["by_reason"].get(r, {"count": 0, "pnl": 0.0})
                print(f"{r:<14} {row['count']:>6} {row['pnl']:>12.6f}")
            print(f"{'closed':<14} {ta['n_closed']:>6} "
                  f"{ta['realized_pnl']:>12.6f}   open {ta['n_open']}, "
                  f"kept {len(trades if fills is None else fills)} of "
                  f"{stats['n_records']} records")
            if args.by_regime:
                print(f"{'regime at entry':<16} {'count':>6} "
                      f"{'win rate':>9} {'pnl':>12}")
                for r in [*REGIMES, "unlabelled"]:
                    row = ta["by_regime"].get(
                        r, {"count": 0, "win_rate": 0.0, "pnl": 0.0})
                    print(f"{r:<16} {row['count']:>6} "
                          f"{row['win_rate']:>9.3f} {row['pnl']:>12.6f}")
            if fills is None:
                path = eng.last_saved.with_name(
                    eng.last_saved.stem + "_trades.csv")
                with open(path, "w", newline="") as f:
                    w = csv.DictWriter(f, fieldnames=[*FIELDS, "duration"])
                    w.writeheader()
                    w.writerows(trades)
                print(f"trades -> {path}")
        return

    if args.cmd == "optimize":
        eng = BacktestEngine(args.data_dir,
                             device="cpu" if args.cpu else None)
        stats = eng.optimize(args.symbol, args.pop, args.generations,
                             args.candles, strategy=args.strategy)
        print(json.dumps(stats, indent=2, default=str))
        return

    if args.cmd == "list":
        eng = BacktestEngine(args.data_dir, device="cpu")
        avail = dm.list_available()
        print(json.dumps({
            "data": avail,
            "results": [
                {k: r.get(k) for k in ("symbol", "strategy", "sharpe",
                                       "total_return_pct", "n_trades")}
                for r in eng.list_results()
            ],
        }, indent=2))
        return

    if args.cmd == "analyze":
        _METRIC_ALIASES = {"sharpe_ratio": "sharpe",
                           "total_return": "total_return_pct",
                           "return": "total_return_pct"}
        eng = BacktestEngine(args.data_dir, device="cpu")
        results = eng.list_results()
        ra = ResultAnalyzer(f"{args.data_dir}/analysis")
        report = ra.summary_report(results)
        if args.metric:
            m = _METRIC_ALIASES.get(args.metric, args.metric)
            best = report.get("best_by", {}).get(m)
            if best is None:
                known = sorted(report.get("best_by", {}))
                raise SystemExit(f"unknown metric {args.metric!r} "
                                 f"(known: {known})")
            print(json.dumps({"metric": m, "best": best,
                              "n_results": report.get("n_results")},
                             indent=2))
        else:
            print(json.dumps(report, indent=2))
        if results:
            p = ra.comparison_chart(results)
            print(f"comparison chart -> {p}")


if __name__ == "__main__":
    main()
