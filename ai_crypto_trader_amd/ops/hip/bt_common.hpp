// What every backtest kernel shares (backtest.hip, backtest_tp.hip,
// backtest_grid.hip, backtest_dca.hip): the block geometry, the 10-slot
// metrics vector with its mark-to-market and finalize formula
// (engine_cpu.finalize_metrics), and the XCD-affine block map — so
// everything downstream of the metrics tensor is family-agnostic and a
// contract change lands in one place.
#pragma once

#include "common.hpp"

#define BT_BLOCK 256
#define BT_TILE 256
#define BT_NMETRIC 10            // == engine_cpu.py NMETRIC
#define BT_FEE 0.001f            // == strategy.py FEE
#define BT_EPS 1e-9f
// float32(sqrt(525600)) EXACTLY (0x44353ee6) — a shorter decimal literal
// rounds to the neighbor 0x44353ee5 and biases every sharpe by 1 ulp
#define BT_ANNUALIZE 0x1.6a7dccp+9f

// max / min as ONE instruction. fmaxf / fminf on a loop-carried or loaded
// value compile to a self-max canonicalisation (v_max_f32 x, x, x, which
// quiets a signalling NaN) plus the max itself; per candle and lane that
// was 7 extra VALU in backtest_kernel. The bare instruction returns the
// same bits as fmaxf / fminf for every operand pair that holds no
// SIGNALLING NaN — including a quiet NaN against a number, where both give
// the number. Arithmetic results are never signalling NaNs, and candle
// inputs are assumed finite, so the call sites below (running maxima and
// minima of prices, equities and averages) qualify. Where the compiler
// already emits one instruction (fmaxf(change, 0.0f) and the like, with a
// folded negate) keep fmaxf.
__device__ __forceinline__ float bt_max(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ float bt_min(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// bt_max against a wave-uniform value (a constant): it sits in a scalar
// register, so the loop holds no VGPR for it
__device__ __forceinline__ float bt_max_uniform(float uniform, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "s"(uniform), "v"(b));
    return r;
}

// a product with a wave-uniform factor, kept in a scalar register likewise
__device__ __forceinline__ float bt_mul_uniform(float uniform, float b)
{
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "s"(uniform), "v"(b));
    return r;
}

// max(x, 0) and max(-x, 0), the negate folded into the instruction: what
// fmaxf(x, 0.0f) and fmaxf(-x, 0.0f) compile to when x is an arithmetic
// result, and also when x was loaded (where fmaxf canonicalises first)
__device__ __forceinline__ float bt_pos_part(float x)
{
    float r;
    asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}

__device__ __forceinline__ float bt_neg_part(float x)
{
    float r;
    asm("v_max_f32 %0, -%1, 0" : "=v"(r) : "v"(x));
    return r;
}

// The ten metrics from scalars (engine_cpu.finalize_metrics semantics).
// A free function because bt_trades_kernel holds the inputs in two
// different waves' registers, not in one BtAccum.
__device__ inline void bt_write_metrics(
    float* __restrict__ out, int T, float equity, float n_trades,
    float wins, float gross_p, float gross_l, float max_dd, float sum_ret,
    float sum_ret2)
{
#pragma clang fp contract(off)
    float n = (float)max(T, 1);
    float mean_r = sum_ret / n;
    float var_r = fmaxf(sum_ret2 / n - mean_r * mean_r, 0.0f);
    float sharpe = mean_r / fmaxf(sqrtf(var_r), BT_EPS) * BT_ANNUALIZE;
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

// equity / trade accounting of one lane
struct BtAccum {
    float equity, max_eq, max_dd;
    float n_trades, wins, gross_p, gross_l;
    float sum_ret, sum_ret2;
    // mark()'s drawdown guard constant: 1 - 2^-23, or 0 (guard off) for
    // an initial equity so small that max_eq * max_dd could be subnormal.
    // max_eq never falls below the initial equity. Wave-uniform.
    float dd_c;

    __device__ void init(float initial_equity)
    {
        // readfirstlane: the select is a vector instruction, and without
        // it the constant would occupy a VGPR through the candle loop
        dd_c = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(
            (initial_equity >= 0x1p-100f) ? 0x1.fffffcp-1f : 0.0f)));
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
        max_eq = bt_max(max_eq, equity);
        // The drawdown quotient only matters on the few candles where it
        // exceeds max_dd, so a division-free test skips it on the others,
        // bit for bit: with m = max_eq, d = max_dd, x = m - equity and
        // g = fl(d * dd_c), a skip needs x <= fl(m * g), and
        //   fl(m * g) <= m * d * (1 - 2^-23) * (1 + 2^-24)^2 < m * d,
        // hence x / m < d; correctly rounded division is monotone and d
        // is representable, so fl(x / m) <= d and the max is a no-op.
        // The two roundings are relative only where no product is
        // subnormal: d is 0 or at least 2^-24 (a positive x = fl(m - e)
        // is at least half an ulp of m), so d * dd_c never is, and m * g
        // is not while m >= 2^-100 — init() switches the guard off below
        // that. d == 0 (or the guard off) gives the threshold 0: only
        // x == 0 skips, where the quotient is 0 too. A NaN in x or in
        // the threshold fails the compare and takes the divide.
        const float x = max_eq - equity;
        if (!(x <= max_eq * bt_mul_uniform(dd_c, max_dd)))
            max_dd = bt_max(max_dd, x / max_eq);
    }

    __device__ void finalize(float* __restrict__ out, int T) const
    {
        bt_write_metrics(out, T, equity, n_trades, wins, gross_p, gross_l,
                         max_dd, sum_ret, sum_ret2);
    }
};

// block -> (symbol, param chunk): same-symbol blocks share an XCD when the
// shape allows (the dispatcher places block b on XCD b%8), so one symbol's
// candle stream stays in one XCD's L2.
__device__ inline void bt_block_map(int bid, int nsym, int chunks_per_sym,
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
