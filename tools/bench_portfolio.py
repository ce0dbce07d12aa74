#!/usr/bin/env python3
"""Portfolio backtest throughput at the flagship shape (pop=1024 x 64
symbols x 2^20 candles, max_positions 8): the flags phase (bt_flags) and
the portfolio phase (bt_portfolio) each alone, the two together through
run_backtest_portfolio_gpu, and, for orientation only, the per-lane
run_backtest_continuous_gpu on the same machine and shape.

Rates are strategy-candles per second, P * nsym * T / time: a host clock
around `iters` back-to-back calls that end in a device synchronise, after
one warm call. A GPU is required.

  python tools/bench_portfolio.py [--pop 1024] [--symbols 64]
      [--candles 1048576] [--max-positions 8] [--iters 5] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=1024)
    ap.add_argument("--symbols", type=int, default=64)
    ap.add_argument("--candles", type=int, default=1 << 20)
    ap.add_argument("--max-positions", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tail", type=int, default=2048)
    ap.add_argument("--out", type=str, default=None,
                    help="also write the JSON here")
    args = ap.parse_args()

    from ai_crypto_trader_amd.backtesting.strategy import random_population
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.ops import require_hip_ops
    from ai_crypto_trader_amd.ops.backtest import (
        _flag_cache, pick_nshards, run_backtest_continuous_gpu,
        run_backtest_portfolio_gpu,
    )

    assert torch.cuda.is_available(), "bench_portfolio needs a GPU"
    dev = torch.device("cuda:0")
    ops = require_hip_ops()

    nsym, T, P = args.symbols, args.candles, args.pop
    c_t = torch.from_numpy(
        candles_chl_v(generate_ohlcv(T, nsym, seed=0))).to(dev)
    p_t = torch.from_numpy(random_population(P, seed=1)).to(dev)
    evals = P * nsym * T
    nshards = min(pick_nshards(nsym, T, P, tail=args.tail),
                  max(1, T // ops.BT_RESNAP))

    def timeit(fn):
        fn()  # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.iters
        return {"s": dt, "gcandles_per_s": evals / dt / 1e9}

    out = {
        "device": torch.cuda.get_device_name(dev),
        "shape": {"pop": P, "nsym": nsym, "T": T,
                  "max_positions": args.max_positions},
        "nshards": nshards, "iters": args.iters,
        "method": "host clock around iters calls ending in a device "
                  "synchronise, after one warm call; rate = P * nsym * T / "
                  "time; seeded synthetic candles and population",
    }

    res = run_backtest_portfolio_gpu(
        c_t, p_t, max_positions=args.max_positions, nshards=nshards,
        tail=args.tail)
    torch.cuda.synchronize()
    out["result"] = {
        "trades_per_strategy": float(res.metrics[:, 1].mean()),
        "refused_slots_per_strategy": float(res.refused[:, 0].float().mean()),
        "refused_cash_per_strategy": float(res.refused[:, 1].float().mean()),
    }
    out["portfolio_end_to_end"] = timeit(lambda: run_backtest_portfolio_gpu(
        c_t, p_t, max_positions=args.max_positions, nshards=nshards,
        tail=args.tail))

    (eflags, xflags, _carry), = _flag_cache.values()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out["flags_phase"] = timeit(lambda: ops.bt_flags(
        c_t.data_ptr(), p_t.data_ptr(), eflags.data_ptr(),
        xflags.data_ptr(), nsym, T, P, nshards, args.tail, 0, nshards,
        stream))
    metrics = torch.empty_like(res.metrics)
    per_symbol = torch.empty_like(res.per_symbol)
    refused = torch.empty_like(res.refused)
    out["portfolio_phase"] = timeit(lambda: ops.bt_portfolio(
        c_t.data_ptr(), p_t.data_ptr(), eflags.data_ptr(),
        xflags.data_ptr(), metrics.data_ptr(), per_symbol.data_ptr(),
        refused.data_ptr(), 0, nsym, T, P, args.max_positions, 1.0, 0, 0,
        stream))
    assert torch.equal(metrics.view(torch.int32),
                       res.metrics.view(torch.int32))

    # orientation only: the per-lane accounts on the same shape
    out["continuous_per_lane_for_orientation"] = timeit(
        lambda: run_backtest_continuous_gpu(c_t, p_t, nshards=nshards,
                                            tail=args.tail))

    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
