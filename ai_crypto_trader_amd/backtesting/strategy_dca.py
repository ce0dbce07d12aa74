"""Dollar-cost-averaging strategy family — the shared CPU/GPU contract.

The reference ships DCA as a live bot (services/dca_strategy.py:347-451
schedules, :817-863 dip buys); services/grid_dca.py::DCAStrategy is its
counterpart here. This module turns the price-driven part of it —
scheduled buys, value averaging, dip buys with a cooldown, and a
take-profit on the average cost that closes the accumulation cycle — into
a deterministic per-candle state machine, so a GA population of DCA
schedules marches through candles as independent GPU lanes. It emits the
same 10-slot metrics vector as the vote machine (backtesting/strategy.py).

A schedule is a flat float32 vector with the layout below, consumed by the
numpy twin (backtesting/engine_dca_cpu.py) and the HIP kernel
(ops/hip/backtest_dca.hip) — keep the three in sync.

Param vector layout (DCA_NPARAM float32 slots):
  0  period             [15, 720] int    candles between scheduled buys
  1  base_order_frac    [0.002, 0.05]    scheduled order, as a fraction of
                                         the INITIAL equity (the role of
                                         DCAConfig.base_order_usd):
                                         base = base_order_frac*initial
  2  dip_threshold_pct  [0.01, 0.2]      dip = close below the rolling
                                         high by this fraction
  3  dip_multiplier     [1.0, 4.0]       order multiplier on a dip
  4  dip_cooldown       [15, 1440] int   candles between dip buys
  5  take_profit_pct    [0.005, 0.2]     exit above the average cost
  6  value_averaging    {0, 1} int       schedule law

One shared, parameter-independent series per symbol (GPU: computed
cooperatively per tile from a DIP_LOOKBACK-candle LDS halo):
  rmax120[t] = max(close[max(0, t-119) .. t])
(the 120 of services/grid_dca.py::DCAStrategy.is_dip).

Arithmetic is f32 with contraction off; omf = 1.0f - FEE. State: cash,
units, invested (all f32), tp_price, the cycle start t0 (0 at the start)
and last_dip (NEVER = -2**20 at the start, so the first dip is free).
dipk = 1 - dip_threshold_pct and tpk = 1 + take_profit_pct are formed once.

Per candle t (both engines implement EXACTLY this order):
  1. if units > 0 and high >= tp_price: sell everything at tp_price:
       proceeds = units*tp_price*omf ; pnl = proceeds - invested
       cash += proceeds ; one trade (n_trades, wins, gross sums as in the
       vote machine) ; units = invested = 0 ; t0 = t+1
       no buy on this candle.
  2. otherwise evaluate a buy, with n = t+1-t0 (>= 1):
       scheduled = n % period == 0
       dip = close < rmax120[t]*dipk and t - last_dip >= dip_cooldown
       neither -> nothing. Else
         usd = base, or if scheduled and value_averaging:
               usd = min(max(base*(float)(n/period) - units*close, 0),
                         4*base)                 (n/period integer)
         on a dip: usd = usd*dip_multiplier ; last_dip = t
         usd = min(usd, cash)
         if usd > 0: cash -= usd ; units += usd*omf/close
                     invested += usd
                     tp_price = invested/units*tpk  (recomputed only here)
  3. mark to market as step 4 of strategy.py: equity = cash + units*close,
     then the return sums and the running-peak drawdown.

Only take-profit exits count as trades, so a schedule that never takes
profit has n_trades == 0 and the no-trade fitness of -1, like a vote
strategy that never enters.

Prices are normalized (close[0] == 1.0); candles are
[close, high, low, volume].
"""

from __future__ import annotations

import numpy as np

from .strategy import FEE  # noqa: F401  (re-exported: the family's fee)

DCA_NPARAM = 7
DIP_LOOKBACK = 120          # rmax120 window (is_dip's recent[-120:])
NEVER = -(1 << 20)          # initial last_dip

DCA_PARAM_NAMES = [
    "period", "base_order_frac", "dip_threshold_pct", "dip_multiplier",
    "dip_cooldown", "take_profit_pct", "value_averaging",
]

# (low, high, is_int) per slot — used by the GA and random init.
DCA_PARAM_BOUNDS = np.array([
    (15, 720, 1), (0.002, 0.05, 0), (0.01, 0.2, 0), (1.0, 4.0, 0),
    (15, 1440, 1), (0.005, 0.2, 0), (0, 1, 1),
], dtype=np.float32)

# ≈ config.DCAConfig defaults (dip 5 % / x2, fixed schedule) with the live
# bot's 60-candle period; 1 % of equity per order, 5 % take-profit.
DCA_DEFAULT_PARAMS = np.array(
    [60, 0.01, 0.05, 2.0, 120, 0.05, 0], dtype=np.float32)


def dca_params_to_dict(vec: np.ndarray) -> dict:
    return {name: float(v) for name, v in zip(DCA_PARAM_NAMES, vec)}


def dict_to_dca_params(d: dict) -> np.ndarray:
    vec = DCA_DEFAULT_PARAMS.copy()
    for i, name in enumerate(DCA_PARAM_NAMES):
        if name in d:
            vec[i] = d[name]
    return vec


def clip_dca_params(pop: np.ndarray) -> np.ndarray:
    """Clip a (pop, DCA_NPARAM) array into bounds; round integer slots."""
    lo = DCA_PARAM_BOUNDS[:, 0]
    hi = DCA_PARAM_BOUNDS[:, 1]
    is_int = DCA_PARAM_BOUNDS[:, 2] > 0
    out = np.clip(pop, lo, hi)
    out[:, is_int] = np.rint(out[:, is_int])
    return out.astype(np.float32)


def random_dca_population(pop_size: int, seed: int = 0) -> np.ndarray:
    """Seeded uniform random population within bounds,
    (pop, DCA_NPARAM) f32."""
    rng = np.random.default_rng(seed)
    lo = DCA_PARAM_BOUNDS[:, 0]
    hi = DCA_PARAM_BOUNDS[:, 1]
    pop = rng.uniform(lo, hi, size=(pop_size, DCA_NPARAM)).astype(
        np.float32)
    return clip_dca_params(pop)


def from_config(cfg) -> np.ndarray:
    """config.DCAConfig -> param vector: the dip threshold and multiplier
    carry over, schedule == "value_averaging" sets slot 6; interval_s is
    wall-clock and base_order_usd an absolute amount, neither of which a
    normalized backtest has, so period and base_order_frac keep their
    defaults."""
    vec = DCA_DEFAULT_PARAMS.copy()
    vec[2] = float(cfg.dip_threshold_pct)
    vec[3] = float(cfg.dip_multiplier)
    vec[6] = 1.0 if cfg.schedule == "value_averaging" else 0.0
    return clip_dca_params(vec[None])[0]
