"""CPU golden twin of the DCA family (numpy, float32).

Implements EXACTLY the per-candle state machine specified in
strategy_dca.py — the reference the HIP kernel
(ops/hip/backtest_dca.hip) is validated against and the engine behind
family="dca" on CPU. Vectorized over lanes = (param-set x symbol); loops
over candles — the same loop order as one GPU lane.
"""

from __future__ import annotations

import numpy as np

from .engine_cpu import NMETRIC, finalize_metrics
from .fills import (
    DEFAULT_MAX_FILLS, KIND_DIP, KIND_SCHEDULED, KIND_SCHEDULED_DIP,
    KIND_TAKE_PROFIT, FillWriter,
)
from .strategy_dca import DCA_NPARAM, DIP_LOOKBACK, FEE, NEVER


def rolling_max_close(candles: np.ndarray) -> np.ndarray:
    """rmax120: max close over min(t+1, DIP_LOOKBACK) candles,
    (nsym, T, 4) -> (nsym, T) f32. Shared by every lane of a symbol."""
    from numpy.lib.stride_tricks import sliding_window_view

    close = candles[:, :, 0]
    nsym = close.shape[0]
    pad = np.full((nsym, DIP_LOOKBACK - 1), -np.inf, close.dtype)
    cp = np.concatenate([pad, close], axis=1)
    return sliding_window_view(cp, DIP_LOOKBACK, axis=1).max(axis=-1)


def run_dca_backtest_cpu(
    candles: np.ndarray,       # (nsym, T, 4) f32 [close, high, low, volume]
    population: np.ndarray,    # (P, DCA_NPARAM) f32
    *,
    initial_equity: float = 1.0,
    record_equity: bool = False,
    record_fills: bool = False,
    max_fills: int = DEFAULT_MAX_FILLS,
    equity_stride: int = 1,
):
    """Run every DCA schedule against every symbol.

    Returns metrics (P, nsym, NMETRIC) f32; optionally the full equity
    curves (P, nsym, T) f32.

    record_fills=True returns a `FillLedger` (backtesting/fills.py)
    instead: the metrics, up to `max_fills` fill records per lane and the
    equity sampled every `equity_stride` candles — the twin of
    ops/hip/backtest_fills.hip's DCA kernel."""
    f32 = np.float32
    candles = np.asarray(candles, dtype=f32)
    population = np.asarray(population, dtype=f32)
    assert candles.ndim == 3 and candles.shape[2] == 4
    assert population.ndim == 2 and population.shape[1] == DCA_NPARAM
    nsym, T, _ = candles.shape
    P = population.shape[0]
    L = P * nsym

    par = np.repeat(population, nsym, axis=0)
    period = np.maximum(par[:, 0].astype(np.int64), 1)
    base = (par[:, 1] * f32(initial_equity)).astype(f32)
    four_base = (f32(4.0) * base).astype(f32)
    dipk = f32(1.0) - par[:, 2]
    dip_mult = par[:, 3]
    cooldown = par[:, 4].astype(np.int64)
    tpk = f32(1.0) + par[:, 5]
    va = par[:, 6] > f32(0.5)
    omf = f32(1.0) - f32(FEE)

    cash = np.full(L, initial_equity, f32)
    units = np.zeros(L, f32)
    invested = np.zeros(L, f32)
    tp_price = np.zeros(L, f32)
    t_start = np.zeros(L, np.int64)            # t0 of the contract
    last_dip = np.full(L, NEVER, np.int64)

    equity = np.full(L, initial_equity, f32)
    max_eq = np.full(L, initial_equity, f32)
    max_dd = np.zeros(L, f32)
    n_trades = np.zeros(L, f32)
    wins = np.zeros(L, f32)
    gross_p = np.zeros(L, f32)
    gross_l = np.zeros(L, f32)
    sum_ret = np.zeros(L, f32)
    sum_ret2 = np.zeros(L, f32)
    curves = np.empty((L, T), f32) if record_equity else None

    close_all = np.ascontiguousarray(candles[:, :, 0])
    high_all = np.ascontiguousarray(candles[:, :, 1])
    rmax_all = np.ascontiguousarray(rolling_max_close(candles))
    sym_idx = np.tile(np.arange(nsym), P)

    fw = None
    if record_fills:
        assert not record_equity, "the ledger carries its own equity samples"
        fw = FillWriter(L, T, max_fills, equity_stride)
        cycle = np.zeros(L, np.int32)          # take-profits so far

    # flat lanes divide 0/0 for a tp_price nobody reads
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            close = close_all[sym_idx, t]
            high = high_all[sym_idx, t]
            rmax = rmax_all[sym_idx, t]

            # --- 1. take profit ------------------------------------------
            tp_hit = (units > 0) & (high >= tp_price)
            proceeds = units * tp_price * omf
            pnl = proceeds - invested
            cash = np.where(tp_hit, cash + proceeds, cash)
            n_trades += tp_hit
            wins += tp_hit & (pnl > 0)
            gross_p += np.where(tp_hit, np.maximum(pnl, f32(0.0)), f32(0.0))
            gross_l += np.where(tp_hit, np.maximum(-pnl, f32(0.0)),
                                f32(0.0))
            if fw is not None and tp_hit.any():
                i = np.flatnonzero(tp_hit)
                fw.put(i, t=t, kind=KIND_TAKE_PROFIT, slot=cycle[i],
                       price=tp_price[i], units=units[i], cash=proceeds[i],
                       pnl=pnl[i], units_held=f32(0.0))
                cycle[i] += 1
            units = np.where(tp_hit, f32(0.0), units)
            invested = np.where(tp_hit, f32(0.0), invested)

            # --- 2. scheduled / dip buy (n from the pre-candle t0) --------
            n = t + 1 - t_start
            sched = ~tp_hit & (n % period == 0)
            dip = (~tp_hit & (close < rmax * dipk)
                   & (t - last_dip >= cooldown))
            nper = (n // period).astype(f32)
            gap = base * nper - units * close
            usd = np.where(
                sched & va,
                np.minimum(np.maximum(gap, f32(0.0)), four_base), base)
            usd = np.where(dip, usd * dip_mult, usd).astype(f32)
            last_dip = np.where(dip, t, last_dip)
            usd = np.minimum(usd, cash)
            buying = (sched | dip) & (usd > 0)
            cash = np.where(buying, cash - usd, cash)
            du = usd * omf / close
            units = np.where(buying, units + du, units)
            invested = np.where(buying, invested + usd, invested)
            tp_price = np.where(buying, invested / units * tpk, tp_price)
            t_start = np.where(tp_hit, t + 1, t_start)
            if fw is not None and buying.any():
                i = np.flatnonzero(buying)
                kind = np.where(
                    dip, np.where(sched, KIND_SCHEDULED_DIP, KIND_DIP),
                    KIND_SCHEDULED)
                fw.put(i, t=t, kind=kind[i], slot=cycle[i], price=close[i],
                       units=du[i], cash=-usd[i], pnl=f32(0.0),
                       units_held=units[i])

            # --- 3. mark to market ---------------------------------------
            new_eq = cash + units * close
            r = new_eq / equity - f32(1.0)
            sum_ret += r
            sum_ret2 += r * r
            equity = new_eq
            max_eq = np.maximum(max_eq, equity)
            max_dd = np.maximum(max_dd, (max_eq - equity) / max_eq)
            if record_equity:
                curves[:, t] = equity
            if fw is not None:
                fw.sample(t, equity)

    metrics = finalize_metrics(
        T, equity, n_trades, wins, gross_p, gross_l, max_dd, sum_ret,
        sum_ret2
    ).reshape(P, nsym, NMETRIC)
    if fw is not None:
        return fw.ledger(metrics, P, nsym)
    if record_equity:
        return metrics, curves.reshape(P, nsym, T)
    return metrics
