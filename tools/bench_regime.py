#!/usr/bin/env python3
"""Regime stack on the GPU: universe detection, long-history labelling and
E-step throughput. Run by hand; writes profiles/regime_universe.json.

    python tools/bench_regime.py [--parts universe,features,estep]
                                 [--symbols 64] [--reps 5] [--out PATH]

universe  S symbols x lookback 500, method hmm, 30 EM iterations.
          New path: MarketRegimeService.detect_many on the device, median
          of --reps timed runs after a warm-up. Baseline: the same symbols
          through the existing per-symbol `detect` in a loop on the device
          (GaussianHMMTorch's per-timestep torch loop), one warm-up symbol
          and then one pass over the universe, every symbol timed.
features  regime_features_gpu on S = 8 x T = 1e6 closes, rows/s (median).
          Baseline: extract_features on the HOST at T = 1e5, one run.
estep     hmm_estep_gpu at B in {64, 1024}, T = 468, K = 4, F = 6,
          sequence-steps/s (median).
Every timing is a host clock around work that ends in a device
synchronise. The file is rewritten after every part."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

DEV = "cuda:0"


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def bench_universe(S, reps):
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.market_regime import (
        MarketRegimeService,
    )

    cfg = AppConfig()
    cfg.regime.method = "hmm"
    lookback = cfg.regime.lookback
    closes = candles_chl_v(generate_ohlcv(lookback, S, seed=5))[:, :, 0]
    uni = {f"S{i}": closes[i].astype(np.float64) for i in range(S)}
    svc = MarketRegimeService(InProcessBus(), cfg, device=DEV)
    res = {}
    new = timed(lambda: res.update(many=svc.detect_many(uni)), reps)
    # baseline: warm up on one symbol, then every symbol once
    svc.detect(uni["S0"])
    torch.cuda.synchronize()
    per_symbol, loop = [], {}
    for sym, c in uni.items():
        t0 = time.perf_counter()
        loop[sym] = svc.detect(c)
        torch.cuda.synchronize()
        per_symbol.append(time.perf_counter() - t0)
        print(f"detect {sym}: {per_symbol[-1]:.3f} s", flush=True)
    same = sum(loop[s][0] == res["many"][s][0] for s in uni)
    return {
        "shape": {"symbols": S, "lookback": lookback, "method": "hmm",
                  "em_iterations": 30, "n_regimes": cfg.regime.n_regimes},
        "detect_many_s": {"median": float(np.median(new)),
                          "min": float(min(new)), "max": float(max(new)),
                          "reps": reps},
        "detect_loop_s": {"total": float(sum(per_symbol)),
                          "per_symbol_median": float(np.median(per_symbol)),
                          "passes": 1},
        "speedup": float(sum(per_symbol) / np.median(new)),
        "same_regime_as_loop": f"{same}/{S}",
    }


def bench_features(reps):
    from ai_crypto_trader_amd.ops.regime import regime_features_gpu
    from ai_crypto_trader_amd.services.market_regime import extract_features

    S, T, win = 8, 1_000_000, 32
    rng = np.random.default_rng(3)
    closes = (100 * np.exp(np.cumsum(rng.normal(0, 1e-3, (S, T)), 1))
              ).astype(np.float32)
    dev = torch.from_numpy(closes).to(DEV)
    out = torch.empty(S * (T - win) * 6, device=DEV)
    inner = 50                      # one launch is too short a window
    lens = torch.full((S,), T, dtype=torch.int32, device=DEV)
    ts = [t / inner for t in timed(
        lambda: [regime_features_gpu(dev, lens, win, out=out)
                 for _ in range(inner)], reps, 1)]
    rows = S * (T - win)
    t0 = time.perf_counter()
    extract_features(closes[0, :100_000].astype(np.float64), win)
    host = time.perf_counter() - t0
    return {
        "shape": {"symbols": S, "T": T, "win": win},
        "gpu_s": {"median": float(np.median(ts)), "min": float(min(ts)),
                  "reps": reps, "launches_per_rep": inner},
        "gpu_rows_per_s": float(rows / np.median(ts)),
        "host_extract_features": {
            "T": 100_000, "seconds": host, "runs": 1,
            "rows_per_s": float((100_000 - win) / host),
            "note": "host CPU only, one symbol, not a GPU figure"},
    }


def bench_estep(reps):
    from ai_crypto_trader_amd.ops.regime import hmm_estep_gpu

    T, K, F = 468, 4, 6
    out = {}
    for B in (64, 1024):
        g = torch.Generator().manual_seed(B)
        X = torch.randn(B, T, F, generator=g).to(DEV)
        mu = torch.randn(B, K, F, generator=g).to(DEV)
        var = torch.ones(B, K, F, device=DEV)
        logA = torch.log(torch.full((B, K, K), 1.0 / K, device=DEV))
        logpi = torch.log(torch.full((B, K), 1.0 / K, device=DEV))
        lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
        inner = 50
        ts = timed(lambda: [hmm_estep_gpu(X, lens, mu, var, logA, logpi)
                            for _ in range(inner)], reps, 1)
        per = float(np.median(ts)) / inner
        out[f"B={B}"] = {"shape": {"B": B, "T": T, "K": K, "F": F},
                         "launch_s": per,
                         "sequence_steps_per_s": B * T / per,
                         "reps": reps, "launches_per_rep": inner}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="universe,features,estep")
    ap.add_argument("--symbols", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/regime_universe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regime needs a GPU: nothing here is "
                         "measured on a CPU")
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    result = json.loads(path.read_text()) if path.exists() else {}
    result["device"] = torch.cuda.get_device_name(0)
    for part in args.parts.split(","):
        if part == "universe":
            result[part] = bench_universe(args.symbols, args.reps)
        elif part == "features":
            result[part] = bench_features(args.reps)
        elif part == "estep":
            result[part] = bench_estep(args.reps)
        else:
            raise SystemExit(f"unknown part {part!r}")
        path.write_text(json.dumps(result, indent=2) + "\n")
        print(json.dumps({part: result[part]}), flush=True)


if __name__ == "__main__":
    main()
