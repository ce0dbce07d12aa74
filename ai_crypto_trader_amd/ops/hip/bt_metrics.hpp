// Equity / trade accounting shared by the strategy-family backtest
// kernels (backtest_grid.hip, backtest_dca.hip): the same 10-slot metrics
// vector, step-4 mark-to-market and finalize formula as backtest.hip /
// engine_cpu.finalize_metrics, so everything downstream of the metrics
// tensor is family-agnostic.
#pragma once

#include "common.hpp"

#define FAM_BLOCK 256
#define FAM_TILE 256
#define FAM_NMETRIC 10
#define FAM_FEE 0.001f           // == strategy.py FEE
#define FAM_EPS 1e-9f
// float32(sqrt(525600)) exactly — see backtest.hip BT_ANNUALIZE
#define FAM_ANNUALIZE 0x1.6a7dccp+9f

struct FamAccum {
    float equity, max_eq, max_dd;
    float n_trades, wins, gross_p, gross_l;
    float sum_ret, sum_ret2;

    __device__ void init(float initial_equity)
    {
        equity = initial_equity; max_eq = initial_equity; max_dd = 0.f;
        n_trades = wins = gross_p = gross_l = 0.f;
        sum_ret = sum_ret2 = 0.f;
    }

    __device__ void trade(float pnl)
    {
        n_trades += 1.0f;
        wins += (pnl > 0.0f) ? 1.0f : 0.0f;
        gross_p += fmaxf(pnl, 0.0f);
        gross_l += fmaxf(-pnl, 0.0f);
    }

    __device__ void mark(float new_eq)
    {
#pragma clang fp contract(off)
        float r = new_eq / equity - 1.0f;
        sum_ret += r;
        sum_ret2 += r * r;
        equity = new_eq;
        max_eq = fmaxf(max_eq, equity);
        max_dd = fmaxf(max_dd, (max_eq - equity) / max_eq);
    }

    __device__ void finalize(float* __restrict__ out, int T) const
    {
#pragma clang fp contract(off)
        float n = (float)max(T, 1);
        float mean_r = sum_ret / n;
        float var_r = fmaxf(sum_ret2 / n - mean_r * mean_r, 0.0f);
        float sharpe = mean_r / fmaxf(sqrtf(var_r), FAM_EPS) * FAM_ANNUALIZE;
        if (!(n_trades > 0.0f)) sharpe = 0.0f;
        float win_rate = wins / fmaxf(n_trades, 1.0f);
        float fitness = (n_trades > 0.0f)
                            ? sharpe + win_rate - 2.0f * max_dd
                            : -1.0f;
        out[0] = equity; out[1] = n_trades; out[2] = wins;
        out[3] = gross_p; out[4] = gross_l; out[5] = max_dd;
        out[6] = sum_ret; out[7] = sum_ret2;
        out[8] = sharpe; out[9] = fitness;
    }
};

// block -> (symbol, param chunk): same-symbol blocks share an XCD when the
// shape allows (the dispatcher places block b on XCD b%8) — the map of
// backtest.hip, so one symbol's candle stream stays in one XCD's L2.
__device__ inline void fam_block_map(int bid, int nsym, int chunks_per_sym,
                                     int& sym, int& chunk)
{
    int nblocks = nsym * chunks_per_sym;
    if ((nsym & 7) == 0 && (nblocks & 7) == 0) {
        int xcd = bid & 7, j = bid >> 3;
        sym = xcd + 8 * (j / chunks_per_sym);
        chunk = j % chunks_per_sym;
    } else {
        sym = bid / chunks_per_sym;
        chunk = bid % chunks_per_sym;
    }
}
