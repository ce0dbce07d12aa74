"""Grid-trading strategy family — the shared CPU/GPU contract.

The reference ships grid trading as a live bot
(services/grid_trading_strategy.py:347-386 level construction, :679-780
fill engine, :781-839 breakout rebalance); services/grid_dca.py is its
counterpart here. This module turns those resting-order semantics into a
deterministic per-candle state machine, so a whole GA population of grids
can march through candles as independent GPU lanes. It emits the same
10-slot metrics vector as the vote machine (backtesting/strategy.py), so
finalize_metrics, metrics_to_stats, the GA loop and the analyzers work on
it unchanged.

A grid is a flat float32 vector with the layout below. The same layout is
consumed by the numpy twin (backtesting/engine_grid_cpu.py) and the HIP
kernel (ops/hip/backtest_grid.hip) — keep the three in sync.

Param vector layout (GRID_NPARAM float32 slots):
  0  half_levels   H   [2, 16] int   2H+1 level prices L[0..2H], 2H slots
                                     (the fill state fits one 32-bit mask)
  1  spacing_pct   s   [0.001, 0.02] distance between adjacent levels
  2  geometric         {0, 1} int    level spacing law
  3  capital_frac      [0.1, 1.0]    share of equity committed at each
                                     (re)build; per-slot budget
                                     b = capital_frac*cash/(float)(2H)
                                     (at a build everything is cash, so
                                     cash == equity)
  4  breakout_pct      [0.0, 0.05]   rebuild band beyond the outer levels

Levels, built outward from the centre c with L[H] = c:
  arithmetic: step = c*s ; L[H+j] = c + (float)j*step
                           L[H-j] = c - (float)j*step
  geometric:  r = 1+s    ; L[H+j] = L[H+j-1]*r ; L[H-j] = L[H-j+1]/r
              (sequential multiply / divide — no pow/exp, so the table is
              bit-reproducible on both sides)
Levels are strictly increasing in k. Slot k (0 <= k < 2H) buys at L[k]
and sells at L[k+1]. Both engines clamp H into [1, MAX_HALF].

Arithmetic is f32 with contraction off; omf = 1.0f - FEE.

Build (at t = 0 and at every rebuild), centre = close:
  b  = capital_frac*cash/(float)(2H)
  u0 = b*omf/close
  slots k >= H: filled at market, u0 units each, flagged "initial"
  slots k <  H: empty (a resting buy at L[k])
  cash -= (float)H*b
  units_total = (double)H*(double)u0            (set exactly)
  up_thr = L[2H]*(1+breakout_pct) ; dn_thr = L[0]*(1-breakout_pct)

A filled slot holds units_k = initial ? u0 : b*omf/L[k] — nothing is
stored per slot; the state is two 32-bit masks plus b, u0 and the table.

Per candle (both engines implement EXACTLY this order). t = 0 is build +
step 4 only. For t >= 1, both masks come from the PRE-candle fill state:
  1. sell = filled & (high >= L[k+1]); applied in ascending k:
       proceeds = units_k*L[k+1]*omf ; pnl = proceeds - b
       cash += proceeds ; units_total -= (double)units_k
       one trade: n_trades += 1, wins += pnl > 0,
       gross_profit += max(pnl, 0), gross_loss += max(-pnl, 0)
       the slot becomes empty
  2. buy = ~filled & (low <= L[k]); applied in descending k, each only
     if cash >= b (b is the same for every slot and cash only falls, so
     "while" and "if" agree):
       cash -= b ; units_total += (double)(b*omf/L[k])
       the slot is filled and loses the initial flag
     A slot fills at most once per candle: what sold in step 1 is not in
     the pre-candle buy mask, what is bought here was not in the sell
     mask — no buy-then-sell within a candle.
  3. breakout: if close > up_thr or close < dn_thr:
       liquidate every filled slot at close, ascending k:
         proceeds = units_k*close*omf ; pnl = proceeds - b ; one trade
         cash += proceeds
       then rebuild centred at close from the new cash.
  4. mark to market, as step 4 of strategy.py:
       equity = cash + (float)units_total*close
       r = equity/prev_equity - 1 ; sum_ret += r ; sum_ret2 += r*r
       max_eq = max(max_eq, equity) ; max_dd = max(max_dd,
                                               (max_eq-equity)/max_eq)
     units_total is an f64 running sum (add on buy, subtract on sell, set
     exactly at build) for the reason the vote machine keeps f64
     Bollinger sums: thousands of f32 +/- of nearly equal terms drift.

Prices are normalized (close[0] == 1.0); candles are
[close, high, low, volume].
"""

from __future__ import annotations

import numpy as np

from .strategy import FEE  # noqa: F401  (re-exported: the family's fee)

GRID_NPARAM = 5
MAX_HALF = 16                  # 2*MAX_HALF slots == one 32-bit mask
MAX_LEVELS = 2 * MAX_HALF + 1  # level-table rows

GRID_PARAM_NAMES = [
    "half_levels", "spacing_pct", "geometric", "capital_frac",
    "breakout_pct",
]

# (low, high, is_int) per slot — used by the GA and random init.
GRID_PARAM_BOUNDS = np.array([
    (2, 16, 1), (0.001, 0.02, 0), (0, 1, 1), (0.1, 1.0, 0),
    (0.0, 0.05, 0),
], dtype=np.float32)

# ≈ config.GridConfig defaults (levels=10, range_pct=0.05, arithmetic)
# with the live bot's 0.5 % breakout band (services/grid_dca.py on_price).
GRID_DEFAULT_PARAMS = np.array(
    [5, 0.01, 0, 0.5, 0.005], dtype=np.float32)


def grid_params_to_dict(vec: np.ndarray) -> dict:
    return {name: float(v) for name, v in zip(GRID_PARAM_NAMES, vec)}


def dict_to_grid_params(d: dict) -> np.ndarray:
    vec = GRID_DEFAULT_PARAMS.copy()
    for i, name in enumerate(GRID_PARAM_NAMES):
        if name in d:
            vec[i] = d[name]
    return vec


def clip_grid_params(pop: np.ndarray) -> np.ndarray:
    """Clip a (pop, GRID_NPARAM) array into bounds; round integer slots."""
    lo = GRID_PARAM_BOUNDS[:, 0]
    hi = GRID_PARAM_BOUNDS[:, 1]
    is_int = GRID_PARAM_BOUNDS[:, 2] > 0
    out = np.clip(pop, lo, hi)
    out[:, is_int] = np.rint(out[:, is_int])
    return out.astype(np.float32)


def random_grid_population(pop_size: int, seed: int = 0) -> np.ndarray:
    """Seeded uniform random population within bounds,
    (pop, GRID_NPARAM) f32."""
    rng = np.random.default_rng(seed)
    lo = GRID_PARAM_BOUNDS[:, 0]
    hi = GRID_PARAM_BOUNDS[:, 1]
    pop = rng.uniform(lo, hi, size=(pop_size, GRID_NPARAM)).astype(
        np.float32)
    return clip_grid_params(pop)


def from_config(cfg) -> np.ndarray:
    """config.GridConfig -> param vector: H = levels//2, s = range_pct/H
    (the live grid spans centre*(1 +- range_pct)), geometric from
    `spacing`, capital_frac = levels*order_size_pct (capped by the
    bounds); the breakout band keeps its default."""
    H = max(int(cfg.levels) // 2, 1)
    vec = GRID_DEFAULT_PARAMS.copy()
    vec[0] = H
    vec[1] = float(cfg.range_pct) / H
    vec[2] = 1.0 if cfg.spacing == "geometric" else 0.0
    vec[3] = float(cfg.levels) * float(cfg.order_size_pct)
    return clip_grid_params(vec[None])[0]
