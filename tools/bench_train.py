#!/usr/bin/env python3
"""Training-workload benchmarks for the BASELINE.json configs beyond the
bench.py headline:

  #2  LSTM price predictor — 32 symbols x 1M 1m-candles resident in HBM,
      bf16 compute, windows (seq 60 x 9 features) sampled on-device,
      full train steps (fwd + bwd + Adam).
  #4  PPO agent — 256 synthetic-market envs stepped by the HIP env
      kernel, GAE on the HIP reverse-scan kernel, full train_step.

  multi  M per-symbol LSTM predictors, stacked (one model-axis launch,
      models/lstm_multi.py) vs the serial per-symbol loop.

  python tools/bench_train.py [--workload lstm|ppo|all]
  python tools/bench_train.py --workload lstm_multi --models 9 --batch 32
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch


def build_features_gpu(candles: torch.Tensor) -> torch.Tensor:
    """(nsym, T, 4) cuda -> (nsym, T, 9) features, all on device
    (the GPU twin of services/neural_network.build_features)."""
    from ai_crypto_trader_amd.ops.indicators import indicators_gpu

    ind = indicators_gpu(candles)                  # (nsym, T, 13)
    close = candles[..., 0]
    ret1 = torch.zeros_like(close)
    ret1[:, 1:] = close[:, 1:] / close[:, :-1] - 1.0
    bb_pos = (close - ind[..., 8]) / torch.clamp(
        ind[..., 7] - ind[..., 8], min=1e-9)
    feats = torch.stack([
        close, candles[..., 1], candles[..., 2], candles[..., 3],
        ind[..., 5] / 100.0, ind[..., 4], bb_pos, ret1 * 100.0,
        ind[..., 9],
    ], dim=-1)
    lo = feats.amin(dim=(0, 1), keepdim=True)
    hi = feats.amax(dim=(0, 1), keepdim=True)
    return (feats - lo) / torch.clamp(hi - lo, min=1e-9)


def bench_lstm_train(nsym=32, T=1_000_000, seq=60, batch=16_384,
                     steps=20, warmup=3, seed=0):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.models.zoo import create_model

    candles = torch.from_numpy(
        candles_chl_v(generate_ohlcv(T, nsym, seed=seed))).cuda()
    feats = build_features_gpu(candles)            # (nsym, T, 9) resident
    close = candles[..., 0]
    target = torch.zeros_like(close)
    target[:, :-1] = (close[:, 1:] / close[:, :-1] - 1.0) * 100.0

    model = create_model("lstm", n_features=9).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    g = torch.Generator(device="cuda").manual_seed(seed)

    def sample_batch():
        s = torch.randint(0, nsym, (batch,), device="cuda", generator=g)
        t0 = torch.randint(0, T - seq - 1, (batch,), device="cuda",
                           generator=g)
        idx = t0[:, None] + torch.arange(seq, device="cuda")[None]
        x = feats[s[:, None], idx]                 # (B, seq, 9)
        y = target[s, t0 + seq]
        return x, y

    def step():
        x, y = sample_batch()
        opt.zero_grad(set_to_none=True)
        loss = ((model(x) - y) ** 2).mean()
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {
        "workload": "lstm_train (BASELINE config #2)",
        "ms_per_step": dt * 1e3,
        "windows_per_sec": batch / dt,
        "cells_per_sec": batch * seq / dt,
        "final_loss": float(loss.detach()),
        "config": {"nsym": nsym, "T": T, "seq": seq, "batch": batch,
                   "dtype": "bf16 (recurrent cells) + f32 master",
                   "resident_bytes": int(feats.numel() * 4 +
                                         candles.numel() * 4)},
    }


def bench_lstm_multi(n_models=9, batch=32, T=20_000, seq=60, steps=20,
                     warmup=3, repeats=3, seed=0):
    """M per-symbol predictors, per-model batch `batch`, full train steps
    (fwd + bwd + Adam) two ways on the same resident windows:
      stacked  one StackedLSTMPricePredictor, one Adam
      serial   M LSTMPricePredictors with M Adams, one after another
    `repeats` alternating timed runs of each; medians and max-min spread
    of aggregate windows/s."""
    import statistics

    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.models.lstm import LSTMPricePredictor
    from ai_crypto_trader_amd.models.lstm_multi import (
        StackedLSTMPricePredictor,
    )

    M = n_models
    candles = torch.from_numpy(
        candles_chl_v(generate_ohlcv(T, M, seed=seed))).cuda()
    feats = build_features_gpu(candles)            # (M, T, 9) resident
    close = candles[..., 0]
    target = torch.zeros_like(close)
    target[:, :-1] = (close[:, 1:] / close[:, :-1] - 1.0) * 100.0

    torch.manual_seed(seed)
    singles = [LSTMPricePredictor(9, seq).cuda() for _ in range(M)]
    stacked = StackedLSTMPricePredictor.from_models(singles)
    opt_stacked = torch.optim.Adam(stacked.parameters(), lr=1e-3)
    opts = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in singles]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = torch.arange(M, device="cuda")[:, None]
    ar = torch.arange(seq, device="cuda")

    def sample_batch():
        t0 = torch.randint(0, T - seq - 1, (M, batch), device="cuda",
                           generator=g)
        x = feats[rows[:, :, None], t0[:, :, None] + ar]   # (M, B, seq, 9)
        y = target[rows, t0 + seq]                         # (M, B)
        return x, y

    def step_stacked():
        x, y = sample_batch()
        opt_stacked.zero_grad(set_to_none=True)
        ((stacked(x) - y) ** 2).mean(dim=1).sum().backward()
        opt_stacked.step()

    def step_serial():
        x, y = sample_batch()
        for m in range(M):
            opts[m].zero_grad(set_to_none=True)
            ((singles[m](x[m]) - y[m]) ** 2).mean().backward()
            opts[m].step()

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return M * batch * steps / (time.perf_counter() - t0)

    for _ in range(warmup):
        step_stacked()
        step_serial()
    runs = {"stacked": [], "serial": []}
    for _ in range(repeats):
        runs["stacked"].append(timed(step_stacked))
        runs["serial"].append(timed(step_serial))
    med = {k: statistics.median(v) for k, v in runs.items()}
    return {
        "workload": "lstm_multi_train",
        "windows_per_sec": med,
        "spread_windows_per_sec": {k: max(v) - min(v)
                                   for k, v in runs.items()},
        "runs_windows_per_sec": runs,
        "ms_per_step": {k: M * batch / v * 1e3 for k, v in med.items()},
        "stacked_over_serial": med["stacked"] / med["serial"],
        "config": {"models": M, "batch": batch, "seq": seq, "T": T,
                   "steps": steps, "warmup": warmup, "repeats": repeats},
    }


def bench_ppo(n_envs=256, horizon=128, steps=6, warmup=2, seed=0,
              use_graph=False):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.models.rl import PPOAgent, TradingVecEnv

    market = torch.from_numpy(
        candles_chl_v(generate_ohlcv(500_000, 16, seed=seed))).cuda()
    env = TradingVecEnv(market, n_envs=n_envs, ep_len=1024, seed=seed)
    env.reset()
    agent = PPOAgent("cuda", seed=seed, use_graph=use_graph)

    for _ in range(warmup):
        agent.train_step(env, horizon)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = {}
    for _ in range(steps):
        stats = agent.train_step(env, horizon)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {
        "workload": "ppo_train (BASELINE config #4, 1-GPU shard)",
        "rollout_graph": agent.use_graph,
        "ms_per_step": dt * 1e3,
        "env_steps_per_sec": n_envs * horizon / dt,
        "stats": stats,
        "config": {"n_envs": n_envs, "horizon": horizon,
                   "note": "DP grad all-reduce engages under torchrun"},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all",
                    choices=["all", "lstm", "ppo", "lstm_multi"])
    ap.add_argument("--models", type=int, default=9,
                    help="lstm_multi: number of per-symbol models")
    ap.add_argument("--batch", type=int, default=32,
                    help="lstm_multi: per-model batch size")
    ap.add_argument("--steps", type=int, default=20,
                    help="lstm_multi: timed steps per run")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    if args.workload in ("all", "lstm"):
        print(json.dumps(bench_lstm_train()), flush=True)
    if args.workload == "lstm_multi":
        print(json.dumps(bench_lstm_multi(args.models, args.batch,
                                          steps=args.steps)), flush=True)
    if args.workload in ("all", "ppo"):
        print(json.dumps(bench_ppo()), flush=True)
        print(json.dumps(bench_ppo(use_graph=True)), flush=True)


if __name__ == "__main__":
    main()
