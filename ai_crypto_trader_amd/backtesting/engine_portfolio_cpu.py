"""CPU twin of the portfolio position machine (numpy, float32): the
contract of backtesting/portfolio.py, vectorised over strategies, looping
over candles and — where the account couples them — over symbols in
ascending index. ops/hip/backtest_portfolio.hip computes the same bits.
"""

from __future__ import annotations

import numpy as np

from .engine_cpu import finalize_metrics, run_backtest_cpu
from .portfolio import (
    PortfolioResult, check_shape, n_portfolio_samples, tree_sum64,
)
from .strategy import FEE, NPARAM, WARMUP


def run_portfolio_from_flags_cpu(
    candles: np.ndarray,       # (nsym, T, 4) f32
    population: np.ndarray,    # (P, NPARAM) f32
    entry_flags: np.ndarray,   # (P, nsym, T) bool
    exit_flags: np.ndarray,    # (P, nsym, T) bool
    *,
    max_positions: int,
    initial_equity: float = 1.0,
    equity_stride: int = 0,
    trace: bool = False,
):
    """Twin of bt_portfolio_kernel, as run_trades_from_flags_cpu is the
    twin of bt_trades_kernel. Returns a PortfolioResult; with trace=True
    also a dict of per-candle (P, T) arrays — `cash` (f32), `n_open` (i32)
    and `equity` (f32), each after the candle's mark — and `exits`, the
    counts of exits by "stop", "tp" and "signal" over the whole run."""
    f32 = np.float32
    candles = np.asarray(candles, dtype=f32)
    population = np.asarray(population, dtype=f32)
    assert candles.ndim == 3 and candles.shape[2] == 4
    assert population.ndim == 2 and population.shape[1] == NPARAM
    nsym, T, _ = candles.shape
    P = population.shape[0]
    max_positions, equity_stride = int(max_positions), int(equity_stride)
    check_shape(nsym, max_positions, equity_stride)
    eflags = np.asarray(entry_flags, bool)
    xflags = np.asarray(exit_flags, bool)
    assert eflags.shape == (P, nsym, T) and xflags.shape == (P, nsym, T)

    size_pct = population[:, 12]
    sl_m = (f32(1.0) - population[:, 13])[:, None]
    tp_m = (f32(1.0) + population[:, 14])[:, None]
    trail_m = (f32(1.0) - population[:, 15])[:, None]
    act_m = (f32(1.0) + population[:, 16])[:, None]
    trail_en = (population[:, 15] > 0)[:, None]
    keep = f32(1.0) - f32(FEE)
    zero = f32(0.0)

    # the account and the portfolio accumulator: (P,)
    cash = np.full(P, initial_equity, f32)
    n_open = np.zeros(P, np.int32)
    equity = np.full(P, initial_equity, f32)
    max_eq = np.full(P, initial_equity, f32)
    max_dd = np.zeros(P, f32)
    n_trades = np.zeros(P, f32)
    wins = np.zeros(P, f32)
    gross_p = np.zeros(P, f32)
    gross_l = np.zeros(P, f32)
    sum_ret = np.zeros(P, f32)
    sum_ret2 = np.zeros(P, f32)
    refused = np.zeros((P, 2), np.int32)

    # positions and per-symbol counters: (P, nsym)
    units = np.zeros((P, nsym), f32)
    in_pos = np.zeros((P, nsym), bool)
    entry_cost = np.zeros((P, nsym), f32)
    entry_price = np.zeros((P, nsym), f32)
    stop = np.zeros((P, nsym), f32)
    tp = np.zeros((P, nsym), f32)
    peak = np.zeros((P, nsym), f32)
    per_symbol = np.zeros((P, nsym, 4), f32)

    n_samples = n_portfolio_samples(T, equity_stride)
    samples = np.empty((P, n_samples), f32) if equity_stride else None
    if trace:
        tr = {"cash": np.empty((P, T), f32),
              "n_open": np.empty((P, T), np.int32),
              "equity": np.empty((P, T), f32),
              "exits": {"stop": 0, "tp": 0, "signal": 0}}

    close_all = np.ascontiguousarray(candles[:, :, 0].T)   # (T, nsym)
    high_all = np.ascontiguousarray(candles[:, :, 1].T)
    low_all = np.ascontiguousarray(candles[:, :, 2].T)

    for t in range(T):
        close = close_all[t][None, :]
        high = high_all[t][None, :]
        low = low_all[t][None, :]

        # --- A. exits: each symbol's own tests, all symbols at once -------
        pos = in_pos
        peak = np.where(pos, np.maximum(peak, high), peak)
        trail_on = pos & trail_en & (peak >= entry_price * act_m)
        stop = np.where(trail_on, np.maximum(stop, peak * trail_m), stop)
        hit_sl = pos & (low <= stop)
        hit_tp = pos & ~hit_sl & (high >= tp)
        hit_sig = pos & ~hit_sl & ~hit_tp & xflags[:, :, t]
        exiting = hit_sl | hit_tp | hit_sig
        if exiting.any():
            price = np.where(hit_sl, stop, np.where(hit_tp, tp, close))
            proceeds = units * price * keep
            pnl = proceeds - entry_cost
            won = exiting & (pnl > 0)
            gain = np.where(exiting, np.maximum(pnl, zero), zero)
            loss = np.where(exiting, np.maximum(-pnl, zero), zero)
            per_symbol[:, :, 0] += exiting
            per_symbol[:, :, 1] += won
            per_symbol[:, :, 2] += gain
            per_symbol[:, :, 3] += loss
            # ... reaching the account in ascending symbol index
            for s in np.nonzero(exiting.any(axis=0))[0]:
                ex = exiting[:, s]
                cash = np.where(ex, cash + proceeds[:, s], cash)
                n_trades += ex
                wins += won[:, s]
                gross_p += gain[:, s]
                gross_l += loss[:, s]
                n_open -= ex
            units = np.where(exiting, zero, units)
            in_pos = pos & ~exiting
            if trace:
                tr["exits"]["stop"] += int(hit_sl.sum())
                tr["exits"]["tp"] += int(hit_tp.sum())
                tr["exits"]["signal"] += int(hit_sig.sum())

        # --- B. entries: flat at the start of the candle, flag set --------
        cand = ~pos & eflags[:, :, t]
        for s in np.nonzero(cand.any(axis=0))[0]:
            c = cand[:, s]
            room = n_open < max_positions
            refused[:, 0] += c & ~room
            cost = np.minimum(size_pct * equity, cash)
            funded = ~(cost <= 0)
            refused[:, 1] += c & room & ~funded
            ent = c & room & funded
            if not ent.any():
                continue
            cl = close[0, s]
            units[:, s] = np.where(ent, cost * keep / cl, units[:, s])
            cash = np.where(ent, cash - cost, cash)
            entry_cost[:, s] = np.where(ent, cost, entry_cost[:, s])
            entry_price[:, s] = np.where(ent, cl, entry_price[:, s])
            stop[:, s] = np.where(ent, cl * sl_m[:, 0], stop[:, s])
            tp[:, s] = np.where(ent, cl * tp_m[:, 0], tp[:, s])
            peak[:, s] = np.where(ent, cl, peak[:, s])
            in_pos[:, s] |= ent
            n_open += ent

        # --- C. mark the account to market ---------------------------------
        held = tree_sum64(np.where(in_pos, units * close, zero))
        new_eq = cash + held
        r = new_eq / equity - f32(1.0)
        sum_ret += r
        sum_ret2 += r * r
        equity = new_eq
        max_eq = np.maximum(max_eq, equity)
        max_dd = np.maximum(max_dd, (max_eq - equity) / max_eq)
        if equity_stride and ((t + 1) % equity_stride == 0 or t == T - 1):
            samples[:, t // equity_stride] = equity
        if trace:
            tr["cash"][:, t] = cash
            tr["n_open"][:, t] = n_open
            tr["equity"][:, t] = equity

    metrics = finalize_metrics(
        T, equity, n_trades, wins, gross_p, gross_l, max_dd, sum_ret,
        sum_ret2)
    res = PortfolioResult(metrics, per_symbol, refused, samples,
                          equity_stride)
    return (res, tr) if trace else res


def vote_flags_cpu(candles: np.ndarray, population: np.ndarray):
    """The vote machine's (entry, exit) planes, (P, nsym, T) bool each, from
    the CPU engine's per-candle vote counts (the planes bt_flags_kernel
    packs): entry = t >= WARMUP and net >= entry_votes, exit = net <=
    -exit_votes (net is 0 before WARMUP)."""
    population = np.asarray(population, np.float32)
    _, nets = run_backtest_cpu(candles, population, record_net=True)
    entry_v = population[:, 10].astype(np.int32)[:, None, None]
    exit_v = population[:, 11].astype(np.int32)[:, None, None]
    warm = np.arange(nets.shape[2]) >= WARMUP
    return (nets >= entry_v) & warm, nets <= -exit_v


def run_portfolio_backtest_cpu(
    candles: np.ndarray,
    population: np.ndarray,
    *,
    max_positions: int,
    initial_equity: float = 1.0,
    equity_stride: int = 0,
) -> PortfolioResult:
    """Votes by run_backtest_cpu, positions by the portfolio machine: the
    twin of ops.backtest.run_backtest_portfolio_gpu."""
    candles = np.asarray(candles, np.float32)
    check_shape(candles.shape[0], int(max_positions), int(equity_stride))
    ef, xf = vote_flags_cpu(candles, population)
    return run_portfolio_from_flags_cpu(
        candles, population, ef, xf, max_positions=max_positions,
        initial_equity=initial_equity, equity_stride=equity_stride)
