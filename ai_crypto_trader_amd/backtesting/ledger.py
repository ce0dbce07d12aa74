"""Trade ledger of the vote backtest: which positions a strategy took,
when, at what price, and why each one closed — the record the reference's
backtester is built around (backtesting/strategy_tester.py:314-357) — plus
the sampled equity curve.

Produced by engine_cpu.run_backtest_cpu(record_trades=True) (numpy) and by
ops.backtest.run_backtest_ledger_gpu (ops/hip/backtest_ledger.hip, torch
tensors); both fill the same `Ledger`.

A record is one position of one (strategy, symbol) lane:

    entry_t      i32  candle index of the entry
    exit_t       i32  candle index of the exit, -1 if still open at T
    reason       i32  index into REASONS
    entry_price  f32  close[entry_t]
    exit_price   f32  stop, tp or close as the state machine filled it;
                      0 if open
    units        f32  units bought at entry
    entry_cost   f32  cash spent at entry
    pnl          f32  the exact proceeds - entry_cost the metrics
                      accumulator got; 0 if open

Records are kept in order, per lane, up to `max_trades`; `n_records` counts
every position the run opened, closed or still open, including those past
capacity (overflow drops the newest). Slots at or above
min(n_records, max_trades) hold -1 in the integer fields and 0 in the float
fields.

`trailing_stop` is a stop exit whose stop is strictly above the initial
entry_price * (1 - stop_loss_pct); the other names are
StrategyTester.Trade.reason's.

Equity sample k is the equity after candle min((k+1)*equity_stride-1, T-1),
for k < ceil(T / equity_stride): stride 1 is the whole curve, and the last
sample is always the final equity.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any

REASONS = ("open", "stop_loss", "take_profit", "signal", "trailing_stop")
INT_FIELDS = ("entry_t", "exit_t", "reason")
FLOAT_FIELDS = ("entry_price", "exit_price", "units", "entry_cost", "pnl")
FIELDS = INT_FIELDS + FLOAT_FIELDS
RECORD_BYTES = 4 * len(FIELDS)
DEFAULT_MAX_TRADES = 4096


def n_equity_samples(T: int, equity_stride: int) -> int:
    return -(-T // equity_stride)


@dataclass
class Ledger:
    """Arrays are numpy (CPU twin) or torch tensors (GPU op) alike."""
    metrics: Any          # (P, nsym, NMETRIC) f32
    n_records: Any        # (P, nsym) i32
    entry_t: Any          # (P, nsym, max_trades) i32
    exit_t: Any
    reason: Any
    entry_price: Any      # (P, nsym, max_trades) f32
    exit_price: Any
    units: Any
    entry_cost: Any
    pnl: Any
    equity: Any           # (P, nsym, n_samples) f32
    equity_stride: int

    @property
    def max_trades(self) -> int:
        return int(self.entry_t.shape[2])

    def n_kept(self, p: int, sym: int) -> int:
        return min(int(self.n_records[p, sym]), self.max_trades)

    def trades(self, p: int, sym: int) -> list[dict]:
        """The lane's records as dicts of plain Python numbers: the field
        names above, `reason` as its name, plus `duration` = exit_t -
        entry_t (candles; of an open position: its exit_t is -1, so
        negative). evaluation.calculate_metrics /
        calculate_advanced_metrics and ResultAnalyzer read them as is."""
        n = self.n_kept(p, sym)
        cols = {}
        for f in FIELDS:
            a = getattr(self, f)[p, sym, :n]
            cols[f] = (a.tolist() if not hasattr(a, "cpu")
                       else a.cpu().tolist())
        out = []
        for k in range(n):
            d = {f: cols[f][k] for f in FIELDS}
            d["reason"] = REASONS[d["reason"]]
            d["duration"] = d["exit_t"] - d["entry_t"]
            out.append(d)
        return out

    def numpy(self) -> "Ledger":
        """Host copy (torch tensors -> numpy); a numpy ledger is returned
        as it is."""
        def host(a):
            return a.cpu().numpy() if hasattr(a, "cpu") else a
        return Ledger(
            host(self.metrics), host(self.n_records),
            *(host(getattr(self, f)) for f in FIELDS),
            host(self.equity), self.equity_stride)
