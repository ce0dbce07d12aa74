"""Fill ledger of the grid and DCA families: which level bought when, what
a breakout liquidated, how a DCA cycle accumulated — the per-order events
the reference's grid and DCA bots log — plus the sampled equity curve. The
sibling of ledger.py: a family fills per level / per order, not one
position at a time, so its record is one fill, not one round trip.

Produced by engine_grid_cpu.run_grid_backtest_cpu(record_fills=True) and
engine_dca_cpu.run_dca_backtest_cpu(record_fills=True) (numpy) and by
ops.backtest_families.run_grid_fills_gpu / run_dca_fills_gpu
(ops/hip/backtest_fills.hip, torch tensors); all fill the same
`FillLedger`.

A record is one fill of one (strategy, symbol) lane:

    t           i32  candle index
    kind        i32  index into FILL_KINDS
    slot        i32  grid: slot k of the contract; DCA: index of the
                     accumulation cycle, 0-based, incremented at each
                     take-profit
    price       f32  the price the state machine filled at (grid: L[k],
                     L[k+1], or close for build and breakout; DCA: close
                     or tp_price)
    units       f32  units bought or sold by this fill
    cash        f32  signed cash flow (grid buy or build: -b; DCA buy:
                     -usd; any sell: +proceeds)
    pnl         f32  sells: the exact value the metrics accumulator got
                     (proceeds - b, proceeds - invested); buys: 0
    units_held  f32  inventory after the fill (grid: (float)units_total;
                     DCA: units)

Grid uses the first four FILL_KINDS, DCA the last four. Within a candle
the records follow the order strategy_grid.py / strategy_dca.py fix: grid
sells ascending k, buys descending k, breakout liquidations ascending k,
then the H market fills of the (re)build ascending k from H (the t = 0
build like any rebuild); DCA writes at most one record per candle.

Two grid kinds carry a units_held of their own. A build fill's is the
running (float)j * u0 up to and including that fill, which on the last one
equals (float)units_total. The state machine does not touch units_total
while a breakout liquidates (the rebuild overwrites it), so a breakout
fill's is the inventory the liquidation started from; the build records
that follow restart the count. A rebuild takes its cash in ONE operation,
cash - (float)H * b, so an exact replay of `cash` subtracts a candle's
build records as that one product, not one by one.

Records are kept in order, per lane, up to `max_fills`; `n_records` counts
every fill, including those past capacity (overflow drops the newest).
Slots at or above min(n_records, max_fills) hold -1 in the integer fields
and 0 in the float fields. Equity samples are ledger.py's: sample k is the
equity after candle min((k+1)*equity_stride-1, T-1).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np

from .ledger import n_equity_samples  # noqa: F401  (the shared definition)

FILL_KINDS = ("buy", "sell", "build", "breakout",
              "scheduled", "dip", "scheduled_dip", "take_profit")
(KIND_BUY, KIND_SELL, KIND_BUILD, KIND_BREAKOUT, KIND_SCHEDULED, KIND_DIP,
 KIND_SCHEDULED_DIP, KIND_TAKE_PROFIT) = range(len(FILL_KINDS))
INT_FIELDS = ("t", "kind", "slot")
FLOAT_FIELDS = ("price", "units", "cash", "pnl", "units_held")
FIELDS = INT_FIELDS + FLOAT_FIELDS
RECORD_BYTES = 4 * len(FIELDS)
DEFAULT_MAX_FILLS = 16384

TRIP_FIELDS = ("entry_t", "exit_t", "reason", "entry_price", "exit_price",
               "units", "entry_cost", "pnl", "duration")


def _trip(entry_t, exit_t, reason, entry_price, exit_price, units,
          entry_cost, pnl) -> dict:
    return {
        "entry_t": int(entry_t), "exit_t": int(exit_t), "reason": reason,
        "entry_price": float(entry_price), "exit_price": float(exit_price),
        "units": float(units), "entry_cost": float(entry_cost),
        "pnl": float(pnl), "duration": int(exit_t) - int(entry_t),
    }


def fold_round_trips(fills: list[dict]) -> list[dict]:
    """One lane's complete fill list -> the trade dicts the analyzers read
    (Ledger.trades' keys). Closed trips come in the order of their closing
    fills; what is still held at T follows with exit_t = -1, reason
    "open", pnl 0.

    Grid: a sell or breakout closes the fill that last filled the same
    slot (a buy or a build); entry_cost is that fill's b. DCA: one trip
    per cycle, from its first buy to its take-profit; entry_cost is the
    cycle's invested (the same f32 running sum the engine keeps) and
    entry_price = invested / units at the exit."""
    f32 = np.float32
    out = []
    held = {}                       # grid: slot -> the fill that filled it
    first, invested, last = None, f32(0.0), None    # DCA cycle in progress
    for f in fills:
        kind = f["kind"]
        if kind in ("buy", "build"):
            held[f["slot"]] = f
        elif kind in ("sell", "breakout"):
            e = held.pop(f["slot"])
            out.append(_trip(e["t"], f["t"], kind, e["price"], f["price"],
                             f["units"], -e["cash"], f["pnl"]))
        elif kind == "take_profit":
            out.append(_trip(first["t"], f["t"], kind,
                             invested / f32(f["units"]), f["price"],
                             f["units"], invested, f["pnl"]))
            first, invested, last = None, f32(0.0), None
        else:                       # a DCA buy
            if first is None:
                first = f
            invested = f32(invested + f32(-f["cash"]))
            last = f
    for k in sorted(held):
        e = held[k]
        out.append(_trip(e["t"], -1, "open", e["price"], 0.0, e["units"],
                         -e["cash"], 0.0))
    if first is not None:
        out.append(_trip(first["t"], -1, "open",
                         invested / f32(last["units_held"]), 0.0,
                         last["units_held"], invested, 0.0))
    return out


@dataclass
class FillLedger:
    """Arrays are numpy (CPU twins) or torch tensors (GPU op) alike."""
    metrics: Any          # (P, nsym, NMETRIC) f32
    n_records: Any        # (P, nsym) i32
    t: Any                # (P, nsym, max_fills) i32
    kind: Any
    slot: Any
    price: Any            # (P, nsym, max_fills) f32
    units: Any
    cash: Any
    pnl: Any
    units_held: Any
    equity: Any           # (P, nsym, n_samples) f32
    equity_stride: int

    @property
    def max_fills(self) -> int:
        return int(self.t.shape[2])

    def n_kept(self, p: int, sym: int) -> int:
        return min(int(self.n_records[p, sym]), self.max_fills)

    def fills(self, p: int, sym: int) -> list[dict]:
        """The lane's records as dicts of plain Python numbers: the field
        names above, `kind` as its name."""
        n = self.n_kept(p, sym)
        cols = {}
        for f in FIELDS:
            a = getattr(self, f)[p, sym, :n]
            cols[f] = (a.tolist() if not hasattr(a, "cpu")
                       else a.cpu().tolist())
        out = []
        for k in range(n):
            d = {f: cols[f][k] for f in FIELDS}
            d["kind"] = FILL_KINDS[d["kind"]]
            out.append(d)
        return out

    def round_trips(self, p: int, sym: int) -> list[dict]:
        """The lane's fills folded into trades (fold_round_trips). Needs
        every fill of the lane: ValueError if it overflowed."""
        n = int(self.n_records[p, sym])
        if n > self.max_fills:
            raise ValueError(
                f"lane ({p}, {sym}) made {n} fills and kept "
                f"{self.max_fills}: round trips need them all, raise "
                "max_fills")
        return fold_round_trips(self.fills(p, sym))

    def numpy(self) -> "FillLedger":
        """Host copy (torch tensors -> numpy); a numpy ledger is returned
        as it is."""
        def host(a):
            return a.cpu().numpy() if hasattr(a, "cpu") else a
        return FillLedger(
            host(self.metrics), host(self.n_records),
            *(host(getattr(self, f)) for f in FIELDS),
            host(self.equity), self.equity_stride)


class FillWriter:
    """The numpy twins' recorder: per-lane append with the capacity rule
    above, and the strided equity samples."""

    def __init__(self, L: int, T: int, max_fills: int, equity_stride: int):
        assert max_fills >= 1 and equity_stride >= 1
        self.max_fills, self.stride, self.T = int(max_fills), \
            int(equity_stride), T
        self.n_rec = np.zeros(L, np.int32)
        self.rec = {f: np.full((L, self.max_fills), -1, np.int32)
                    for f in INT_FIELDS}
        self.rec.update({f: np.zeros((L, self.max_fills), np.float32)
                         for f in FLOAT_FIELDS})
        self.eq = np.empty((L, n_equity_samples(T, self.stride)),
                           np.float32)

    def put(self, idx, **vals):
        """Append one record to each lane of `idx` (values are scalars or
        arrays parallel to idx); count it either way."""
        if len(idx) == 0:
            return
        room = self.n_rec[idx] < self.max_fills
        keep = idx[room]
        slot = self.n_rec[keep]
        for f, v in vals.items():
            self.rec[f][keep, slot] = v[room] if np.ndim(v) else v
        self.n_rec[idx] += 1

    def sample(self, t: int, equity):
        if (t + 1) % self.stride == 0 or t == self.T - 1:
            self.eq[:, t // self.stride] = equity

    def ledger(self, metrics, P: int, nsym: int) -> FillLedger:
        return FillLedger(
            metrics, self.n_rec.reshape(P, nsym),
            *(self.rec[f].reshape(P, nsym, self.max_fills) for f in FIELDS),
            self.eq.reshape(P, nsym, -1), self.stride)
