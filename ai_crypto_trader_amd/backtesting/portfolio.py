"""The portfolio position machine: ONE strategy trading a basket of symbols
from ONE cash account, with a cap on concurrent positions — how the live
stack trades (services/trade_executor.py: one quote-asset balance, a
max-positions limit), where every other backtest path gives each
(strategy, symbol) lane a private account.

It is a second consumer of the vote machine's entry / exit flags
(strategy.py steps 1-2, bt_flags_kernel's bitmaps). Implemented twice,
bit for bit: engine_portfolio_cpu.py (numpy twin) and
ops/hip/backtest_portfolio.hip (one wave per strategy, lane = symbol).

Inputs
  candles (nsym, T, 4) f32, population (P, NPARAM) f32 (strategy.py
  layout, unchanged), max_positions in [1, nsym], initial_equity, and per
  (strategy, symbol, candle) the flags
      entry = t >= WARMUP and net >= entry_votes
      exit  = net <= -exit_votes
  1 <= nsym <= MAX_SYMBOLS (one wave lane per symbol).

State per strategy
  cash, n_open and one equity / trade accumulator for the portfolio
  (equity, max_eq, max_dd, n_trades, wins, gross_p, gross_l, sum_ret,
  sum_ret2); per symbol the position (units, in_pos, entry_cost,
  entry_price, stop, tp, peak) and four counters of the symbol's own exits
  (n_trades, wins, gross_p, gross_l).

Per candle t, in this order (f32, no fused multiply-add):

  A. Exits. Every symbol in position runs strategy.py step 3 unchanged:
     peak = max(peak, high); the trailing stop ratchets once peak has
     reached entry_price * (1 + trailing_act_pct); then low <= stop fills
     at the stop, else high >= tp fills at tp, else the exit flag fills at
     the close. proceeds = units * price * (1 - FEE), pnl = proceeds -
     entry_cost. The candle's exits reach the account in ASCENDING SYMBOL
     INDEX, each as one `cash += proceeds`, one trade(pnl) on the portfolio
     accumulator and n_open -= 1 (f32 addition does not associate, so the
     order is part of the contract).

  B. Entries. Candidates are the symbols that were flat when the candle
     began and whose entry flag is set — a symbol that exited in A is not
     one (the single-symbol machine's `else if`). They are taken in
     ASCENDING SYMBOL INDEX:
       - n_open == max_positions: this candidate and every later one of
         the candle is refused for slots (refused[0] += 1 each);
       - cost = min(position_size_pct * equity, cash), `equity` being the
         portfolio equity of the previous mark. cost <= 0: the candidate is
         refused for cash (refused[1] += 1), nothing else changes;
       - otherwise units = cost * (1 - FEE) / close, cash -= cost,
         entry_cost = cost, entry_price = close, stop = close * (1 -
         stop_loss_pct), tp = close * (1 + take_profit_pct), peak = close,
         n_open += 1.
     Cash freed by the exits of A is available here.

  C. Mark. held = sum over symbols of units_s * close_s, a flat symbol
     contributing +0.0. The sum is the BALANCED BINARY TREE over the symbol
     index padded with +0.0 to 64 elements: level k (k = 0..5) replaces
     element i by x[i] + x[i ^ (1 << k)], i.e.
         level 0: (x0 + x1), (x2 + x3), ..., (x62 + x63)
         level 1: ((x0 + x1) + (x2 + x3)), ...
         ...
         level 5: the two 32-element halves
     — what a 6-step cross-lane xor reduction computes in every lane, and
     what `tree_sum64` below computes with six pairwise f32 additions. Then
     the accumulator marks cash + held exactly as strategy.py step 4:
     r = new_eq / equity - 1, sum_ret += r, sum_ret2 += r * r, equity,
     max_eq, max_dd. With nsym == 1 this is cash + units * close bit for
     bit, and the whole machine is the single-symbol one.

Outputs
  metrics    (P, NMETRIC) f32   engine_cpu.finalize_metrics of the
                                portfolio accumulator
  per_symbol (P, nsym, 4) f32   n_trades, wins, gross_p, gross_l of each
                                symbol's own exits
  refused    (P, 2) i32         entry candidates left untaken for slots,
                                for cash
  equity     (P, ceil(T / equity_stride)) f32, or None with
                                equity_stride == 0: the trade ledger's
                                sampling (ledger.py) — sample k is the
                                equity after candle
                                min((k + 1) * equity_stride - 1, T - 1)
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np

from .ledger import n_equity_samples

MAX_SYMBOLS = 64        # one wave: a lane per symbol
PER_SYMBOL_FIELDS = ("n_trades", "wins", "gross_profit", "gross_loss")
REFUSED_FIELDS = ("refused_slots", "refused_cash")


def check_shape(nsym: int, max_positions: int, equity_stride: int) -> None:
    if not 1 <= nsym <= MAX_SYMBOLS:
        raise ValueError(
            f"a portfolio holds 1 to {MAX_SYMBOLS} symbols, not {nsym}")
    if not 1 <= max_positions <= nsym:
        raise ValueError(
            f"max_positions must be in [1, nsym = {nsym}], "
            f"not {max_positions}")
    if equity_stride < 0:
        raise ValueError(f"equity_stride {equity_stride} < 0")


def n_portfolio_samples(T: int, equity_stride: int) -> int:
    return n_equity_samples(T, equity_stride) if equity_stride > 0 else 0


def tree_sum64(x: np.ndarray) -> np.ndarray:
    """Step C's sum over the last axis (length <= 64), f32: pad with +0.0
    to 64, then six levels of adjacent-pair additions."""
    x = np.asarray(x, np.float32)
    n = x.shape[-1]
    assert 1 <= n <= MAX_SYMBOLS
    v = np.zeros(x.shape[:-1] + (MAX_SYMBOLS,), np.float32)
    v[..., :n] = x
    for _ in range(6):
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


@dataclass
class PortfolioResult:
    """Arrays are numpy (CPU twin) or torch tensors (GPU op) alike."""
    metrics: Any          # (P, NMETRIC) f32
    per_symbol: Any       # (P, nsym, 4) f32
    refused: Any          # (P, 2) i32
    equity: Any           # (P, n_samples) f32, or None
    equity_stride: int

    def numpy(self) -> "PortfolioResult":
        def host(a):
            return a.cpu().numpy() if hasattr(a, "cpu") else a
        return PortfolioResult(
            host(self.metrics), host(self.per_symbol), host(self.refused),
            None if self.equity is None else host(self.equity),
            self.equity_stride)
