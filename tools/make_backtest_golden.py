#!/usr/bin/env python3
"""Generate tests/golden/backtest_lane_loop.npz: all 10 metrics of
run_backtest_gpu for the cases of tests/test_gpu_backtest_lane_loop.py.

The file pins what backtest_kernel computed BEFORE its lane loop was
shortened (no self-max canonicalisation, seeded EMAs, one LDS record per
candle, trailing trigger at entry, warm-up loop). It must therefore be
written by the build of the commit that precedes that change, on a GPU,
and never by the code under test: regenerating it with a later build
turns the test into a comparison of the kernel with itself. It holds
outputs only; the test rebuilds the inputs from the seeds below.

    python tools/make_backtest_golden.py            # needs a GPU
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

GOLDEN = (Path(__file__).resolve().parent.parent / "tests" / "golden"
          / "backtest_lane_loop.npz")

NSYM = 3
P_LANES = 70          # one full wave plus a 6-lane wave
# a single candle; the warm-up boundary from both sides (WARMUP = 128);
# the first voting candle; remainders of 1, 2, 3 and 5 candles after the
# 256-candle tile boundary; the ragged 28-candle sub-tile of 700
T_CASES = (1, 127, 128, 129, 131, 257, 258, 259, 261, 700)
# price levels orders of magnitude apart: a seed taken from the wrong
# symbol or the wrong candle cannot pass
SYM_SCALE = (1.0, 37.0, 0.01)
# chosen on the CPU (engine_cpu.run_backtest_cpu): trades happen at
# T = 700, and in the trailing case the trailing stop changes them
MARKET_SEED = 31
MARKET_SIGMA = 2.0
POP_SEED = 17
TRAIL_MARKET_SEED = 7
TRAIL_POP_SEED = 23
TRAIL_T = 700
TRAIL_P = 64
RESNAP_MARKET_SEED = 5
RESNAP_POP_SEED = 3
RESNAP_P = 64
RESNAP_EXTRA = 600    # candles past the first resnap boundary


def market(T, nsym, seed, sigma=MARKET_SIGMA):
    """(nsym, T, 4) candles; close/high/low of symbol s scaled by
    SYM_SCALE[s] (volume is not read by the vote family)."""
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    c = candles_chl_v(generate_ohlcv(T, nsym, seed=seed, sigma=sigma))
    for s in range(nsym):
        c[s, :, :3] *= np.float32(SYM_SCALE[s % len(SYM_SCALE)])
    return np.ascontiguousarray(c)


def population(P, seed):
    """Random strategies with eager entry/exit votes, so that the short
    histories trade."""
    from ai_crypto_trader_amd.backtesting.strategy import random_population
    pop = random_population(P, seed=seed)
    pop[:, 10] = 1.0 + (np.arange(P) % 2)
    pop[:, 11] = 1.0 + ((np.arange(P) // 2) % 2)
    return pop


def trailing_population(P, seed):
    """Even lanes trail (a stop a few candle-sigmas wide that arms after
    a fraction of one), odd lanes have the trailing stop off."""
    pop = population(P, seed)
    rng = np.random.default_rng(seed + 1)
    even = (np.arange(P) % 2) == 0
    pop[:, 13] = 0.05                              # a stop loss out of reach
    pop[:, 14] = 0.2                               # ... and the take profit
    pop[:, 15] = np.where(even, rng.uniform(0.002, 0.008, P), 0.0)
    pop[:, 16] = rng.uniform(0.0005, 0.002, P)
    return pop.astype(np.float32)


def cases():
    """name -> (market, population), rebuilt from the seeds."""
    from ai_crypto_trader_amd.backtesting.strategy import RESNAP
    out = {}
    full = market(max(T_CASES), NSYM, MARKET_SEED)
    pop = population(P_LANES, POP_SEED)
    for T in T_CASES:
        # prefixes of one market: the same candles end at different T
        out[f"T{T}"] = (np.ascontiguousarray(full[:, :T]), pop)
    out["trailing"] = (market(TRAIL_T, NSYM, TRAIL_MARKET_SEED),
                       trailing_population(TRAIL_P, TRAIL_POP_SEED))
    out["resnap"] = (market(RESNAP + RESNAP_EXTRA, 1, RESNAP_MARKET_SEED),
                     population(RESNAP_P, RESNAP_POP_SEED))
    return out


def main():
    import torch

    from ai_crypto_trader_amd.ops.backtest import run_backtest_gpu

    assert torch.cuda.is_available(), "the golden comes from the GPU kernel"
    dev = torch.device("cuda:0")
    out = {}
    for name, (mkt, pop) in cases().items():
        got = run_backtest_gpu(torch.from_numpy(mkt).to(dev),
                               torch.from_numpy(pop).to(dev))
        torch.cuda.synchronize()
        out[name] = got.cpu().numpy()
        print(f"{name}: {out[name].shape} trades={out[name][..., 1].sum():.0f}")
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
