"""CPU golden twin of the grid family (numpy, float32).

Implements EXACTLY the per-candle state machine specified in
strategy_grid.py — the reference the HIP kernel
(ops/hip/backtest_grid.hip) is validated against and the engine behind
family="grid" on CPU. Vectorized over lanes = (param-set x symbol); loops
over candles, and over slots in the order the contract states (sells
ascending, buys descending, liquidation ascending) — the order one GPU
lane applies them in. Slots in which no lane trades on a candle are
skipped, which changes nothing: an untouched lane is a no-op.
"""

from __future__ import annotations

import numpy as np

from .engine_cpu import NMETRIC, finalize_metrics
from .fills import (
    DEFAULT_MAX_FILLS, KIND_BREAKOUT, KIND_BUILD, KIND_BUY, KIND_SELL,
    FillWriter,
)
from .strategy_grid import FEE, GRID_NPARAM, MAX_HALF, MAX_LEVELS

NSLOT = 2 * MAX_HALF


def run_grid_backtest_cpu(
    candles: np.ndarray,       # (nsym, T, 4) f32 [close, high, low, volume]
    population: np.ndarray,    # (P, GRID_NPARAM) f32
    *,
    initial_equity: float = 1.0,
    record_equity: bool = False,
    record_fills: bool = False,
    max_fills: int = DEFAULT_MAX_FILLS,
    equity_stride: int = 1,
):
    """Run every grid against every symbol.

    Returns metrics (P, nsym, NMETRIC) f32; optionally the full equity
    curves (P, nsym, T) f32.

    record_fills=True returns a `FillLedger` (backtesting/fills.py)
    instead: the metrics, up to `max_fills` fill records per lane and the
    equity sampled every `equity_stride` candles — the twin of
    ops/hip/backtest_fills.hip's grid kernel."""
    f32 = np.float32
    f64 = np.float64
    candles = np.asarray(candles, dtype=f32)
    population = np.asarray(population, dtype=f32)
    assert candles.ndim == 3 and candles.shape[2] == 4
    assert population.ndim == 2 and population.shape[1] == GRID_NPARAM
    nsym, T, _ = candles.shape
    P = population.shape[0]
    L = P * nsym

    # lane l = (param p, symbol s), s fastest
    par = np.repeat(population, nsym, axis=0)
    H = np.clip(par[:, 0].astype(np.int32), 1, MAX_HALF)
    twoH = 2 * H
    Hf = H.astype(f32)
    twoHf = twoH.astype(f32)
    s = par[:, 1]
    geo = par[:, 2] > f32(0.5)
    cf = par[:, 3]
    up_k = f32(1.0) + par[:, 4]
    dn_k = f32(1.0) - par[:, 4]
    omf = f32(1.0) - f32(FEE)

    slots = np.arange(NSLOT)
    valid = slots[None, :] < twoH[:, None]              # (L, NSLOT)
    lev = np.zeros((L, MAX_LEVELS), f32)                # level table
    l_buy = lev[:, :NSLOT]                              # L[k]   (views)
    l_sell = lev[:, 1:]                                 # L[k+1]
    filled = np.zeros((L, NSLOT), bool)
    initial = np.zeros((L, NSLOT), bool)
    b = np.zeros(L, f32)
    bomf = np.zeros(L, f32)
    u0 = np.zeros(L, f32)
    up_thr = np.zeros(L, f32)
    dn_thr = np.zeros(L, f32)
    cash = np.full(L, initial_equity, f32)
    units_total = np.zeros(L, f64)

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
    low_all = np.ascontiguousarray(candles[:, :, 2])
    sym_idx = np.tile(np.arange(nsym), P)

    fw = None
    if record_fills:
        assert not record_equity, "the ledger carries its own equity samples"
        fw = FillWriter(L, T, max_fills, equity_stride)

    def build(idx, c, t):
        """(Re)build the grids of lanes `idx` centred at their close `c`."""
        h, th = H[idx], twoH[idx]
        bb = (cf[idx] * cash[idx] / twoHf[idx]).astype(f32)
        bo = (bb * omf).astype(f32)
        uu = (bo / c).astype(f32)
        b[idx], bomf[idx], u0[idx] = bb, bo, uu
        cash[idx] = cash[idx] - Hf[idx] * bb
        units_total[idx] = h.astype(f64) * uu.astype(f64)
        lev[idx, h] = c
        up = c.copy()
        dn = c.copy()
        g = geo[idx]
        r = (f32(1.0) + s[idx]).astype(f32)
        step = (c * s[idx]).astype(f32)
        for j in range(1, MAX_HALF + 1):
            m = j <= h
            if not m.any():
                break
            up = np.where(g, up * r, c + f32(j) * step).astype(f32)
            dn = np.where(g, dn / r, c - f32(j) * step).astype(f32)
            lev[idx[m], h[m] + j] = up[m]
            lev[idx[m], h[m] - j] = dn[m]
            if fw is not None:         # market fill of slot H + j - 1
                fw.put(idx[m], t=t, kind=KIND_BUILD, slot=h[m] + j - 1,
                       price=c[m], units=uu[m], cash=-bb[m], pnl=f32(0.0),
                       units_held=f32(j) * uu[m])
        fl = valid[idx] & (slots[None, :] >= h[:, None])
        filled[idx] = fl
        initial[idx] = fl
        up_thr[idx] = lev[idx, th] * up_k[idx]
        dn_thr[idx] = lev[idx, 0] * dn_k[idx]

    def slot_units(k):
        return np.where(initial[:, k], u0, bomf / l_buy[:, k]).astype(f32)

    def book_trade(m, pnl):
        nonlocal n_trades, wins, gross_p, gross_l
        n_trades += m
        wins += m & (pnl > 0)
        gross_p += np.where(m, np.maximum(pnl, f32(0.0)), f32(0.0))
        gross_l += np.where(m, np.maximum(-pnl, f32(0.0)), f32(0.0))

    all_lanes = np.arange(L)
    # unused table rows stay 0, so bomf/L[k] divides by zero in columns a
    # lane does not own; those results are masked out by `valid`
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            close = close_all[sym_idx, t]
            if t == 0:
                build(all_lanes, close, t)
            else:
                high = high_all[sym_idx, t]
                low = low_all[sym_idx, t]
                # both masks from the pre-candle fill state
                sell = filled & valid & (high[:, None] >= l_sell)
                buy = ~filled & valid & (low[:, None] <= l_buy)
                # --- 1. sells, ascending k -------------------------------
                for k in np.flatnonzero(sell.any(axis=0)):
                    m = sell[:, k]
                    uk = slot_units(k)
                    proceeds = uk * l_sell[:, k] * omf
                    cash = np.where(m, cash + proceeds, cash)
                    units_total = np.where(
                        m, units_total - uk.astype(f64), units_total)
                    book_trade(m, proceeds - b)
                    filled[:, k] &= ~m
                    if fw is not None:
                        i = np.flatnonzero(m)
                        fw.put(i, t=t, kind=KIND_SELL, slot=k,
                               price=l_sell[i, k], units=uk[i],
                               cash=proceeds[i], pnl=(proceeds - b)[i],
                               units_held=units_total[i].astype(f32))
                # --- 2. buys, descending k -------------------------------
                for k in np.flatnonzero(buy.any(axis=0))[::-1]:
                    m = buy[:, k] & (cash >= b)
                    uk = (bomf / l_buy[:, k]).astype(f32)
                    cash = np.where(m, cash - b, cash)
                    units_total = np.where(
                        m, units_total + uk.astype(f64), units_total)
                    filled[:, k] |= m
                    initial[:, k] &= ~m
                    if fw is not None:
                        i = np.flatnonzero(m)
                        fw.put(i, t=t, kind=KIND_BUY, slot=k,
                               price=l_buy[i, k], units=uk[i], cash=-b[i],
                               pnl=f32(0.0),
                               units_held=units_total[i].astype(f32))
                # --- 3. breakout: liquidate at close, rebuild ------------
                brk = (close > up_thr) | (close < dn_thr)
                if brk.any():
                    liq = filled & brk[:, None]
                    for k in np.flatnonzero(liq.any(axis=0)):
                        m = liq[:, k]
                        uk = slot_units(k)
                        proceeds = uk * close * omf
                        cash = np.where(m, cash + proceeds, cash)
                        book_trade(m, proceeds - b)
                        if fw is not None:
                            i = np.flatnonzero(m)
                            fw.put(i, t=t, kind=KIND_BREAKOUT, slot=k,
                                   price=close[i], units=uk[i],
                                   cash=proceeds[i], pnl=(proceeds - b)[i],
                                   units_held=units_total[i].astype(f32))
                    idx = np.flatnonzero(brk)
                    build(idx, close[idx], t)

            # --- 4. mark to market ---------------------------------------
            new_eq = cash + units_total.astype(f32) * close
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
