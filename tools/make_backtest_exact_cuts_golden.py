#!/usr/bin/env python3
"""Generate tests/golden/backtest_exact_cuts.npz: what the backtest kernels
computed for the cases of tests/test_gpu_backtest_exact_cuts.py BEFORE the
drawdown divide in BtAccum::mark got its division-free guard and the candle
record its stochastic / Williams vote thresholds.

All 10 metrics of run_backtest_gpu for three markets x three initial
equities, and of the grid and DCA kernels on the falling market. The file
must be written on a GPU by the build of the commit that precedes those
changes, never by the code under test: regenerating it with a later build
turns the test into a comparison of the kernels with themselves. It holds
outputs only; the test rebuilds the inputs from the seeds below.

    python tools/make_backtest_exact_cuts_golden.py            # needs a GPU
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

GOLDEN = (Path(__file__).resolve().parent.parent / "tests" / "golden"
          / "backtest_exact_cuts.npz")

NSYM = 3
P_LANES = 70          # one full wave plus a 6-lane wave
T = 700               # two 256-candle tiles and a ragged 28-candle sub-tile
EQUITIES = (1e-3, 1.0, 1e4)
POP_SEED = 17
LANE_LOOP_SEED = 31   # the market of tools/make_backtest_golden.py
FALL_SEED = 41
FALL_FROM, FALL_TO = 120, 640   # the slide: 520 candles
FALL_RATE = 0.002               # per candle, against a sigma of 0.0028
FLAT_SEED = 43
FLAT_PERIOD, FLAT_AT, FLAT_LEN = 100, 35, 40
FAMILY_SEED = 11
SYM_SCALE = (1.0, 37.0, 0.01)


def _gbm(seed):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(T, NSYM, seed=seed, sigma=2.0))


def _scaled(c):
    for s in range(NSYM):
        c[s, :, :3] *= np.float32(SYM_SCALE[s])
    return np.ascontiguousarray(c)


def lane_loop_market():
    return _scaled(_gbm(LANE_LOOP_SEED))


def falling_market():
    """A seeded GBM whose close, high and low slide by FALL_RATE a candle
    from FALL_FROM to FALL_TO: positions opened on the way down keep
    setting new maximum drawdowns."""
    c = _gbm(FALL_SEED)
    t = np.clip(np.arange(T) - FALL_FROM, 0, FALL_TO - FALL_FROM)
    c[:, :, :3] *= np.exp(-FALL_RATE * t).astype(np.float32)[None, :, None]
    return _scaled(c)


def flat_market():
    """A seeded GBM with a FLAT_LEN-candle stretch of high == low == close
    in every FLAT_PERIOD candles: the 14-candle range collapses to the
    epsilon floor, close == lmin == hmax, and the equity of a lane in
    position stands still (x == 0 candle after candle)."""
    c = _gbm(FLAT_SEED)
    for t0 in range(FLAT_AT, T, FLAT_PERIOD):
        c[:, t0:t0 + FLAT_LEN, :3] = c[:, t0:t0 + 1, 0:1]
    return _scaled(c)


MARKETS = {"lane_loop": lane_loop_market, "falling": falling_market,
           "flat": flat_market}


def population():
    """Random strategies with eager entry/exit votes, so that 700 candles
    trade."""
    from ai_crypto_trader_amd.backtesting.strategy import random_population
    pop = random_population(P_LANES, seed=POP_SEED)
    pop[:, 10] = 1.0 + (np.arange(P_LANES) % 2)
    pop[:, 11] = 1.0 + ((np.arange(P_LANES) // 2) % 2)
    return pop


def eq_name(eq):
    return f"{eq:g}"


def vote_cases():
    """name -> (market, population, initial_equity)."""
    pop = population()
    return {f"{m}_eq{eq_name(eq)}": (make(), pop, eq)
            for m, make in MARKETS.items() for eq in EQUITIES}


def family_cases():
    """name -> (family, market, population) on the falling market."""
    from ai_crypto_trader_amd.backtesting.families import FAMILIES
    mkt = falling_market()
    return {f"{name}_falling": (fam, mkt,
                                fam.random_population(P_LANES, FAMILY_SEED))
            for name, fam in FAMILIES.items() if name in ("grid", "dca")}


def main():
    import torch

    from ai_crypto_trader_amd.ops.backtest import run_backtest_gpu

    assert torch.cuda.is_available(), "the golden comes from the GPU kernels"
    dev = torch.device("cuda:0")
    out = {}
    for name, (mkt, pop, eq) in vote_cases().items():
        got = run_backtest_gpu(torch.from_numpy(mkt).to(dev),
                               torch.from_numpy(pop).to(dev),
                               initial_equity=eq)
        torch.cuda.synchronize()
        out[name] = got.cpu().numpy()
    for name, (fam, mkt, pop) in family_cases().items():
        got = fam.run_gpu(torch.from_numpy(mkt).to(dev),
                          torch.from_numpy(pop).to(dev))
        torch.cuda.synchronize()
        out[name] = got.cpu().numpy()
    for name, a in out.items():
        print(f"{name}: {a.shape} trades={a[..., 1].sum():.0f} "
              f"max_dd<={a[..., 5].max():.4f}")
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
