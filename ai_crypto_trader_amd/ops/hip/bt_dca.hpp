// The DCA family's per-lane state machine and tile staging
// (backtesting/strategy_dca.py is the contract), shared by
// backtest_dca.hip (metrics only) and backtest_fills.hip (metrics plus
// one record per order). Why rmax120 is computed cooperatively per tile
// and the schedule is a counter pair: backtest_dca.hip's header.
//
// Recorder: step() takes a compile-time recorder and calls
// rec.take_profit() / rec.buy() once per order, at most one per candle
// (backtesting/fills.py has the record). What the recorder needs to
// remember — the cycle index — is the recorder type's own state, not the
// lane's. DcaNoFills has empty inline hooks, whose arguments are values
// the state machine computes anyway, so backtest_dca_kernel compiles to
// what it was before the hooks existed.
#pragma once

#include "bt_common.hpp"

#define DC_NPARAM 7
#define DC_LOOKBACK 120          // == strategy_dca.py DIP_LOOKBACK
#define DC_HALO 128              // >= DC_LOOKBACK - 1
#define DC_SPAN (BT_TILE + DC_HALO)
#define DC_NEVER (-(1 << 20))    // == strategy_dca.py NEVER

namespace {

struct DcaNoFills {
    __device__ __forceinline__ void take_profit(int, float, float, float,
                                                float) {}
    __device__ __forceinline__ void buy(int, bool, bool, float, float, float,
                                        float) {}
};

struct DcaLane {
    // params
    int period, cooldown;
    float base, four_base, dipk, dip_mult, tpk;
    bool va;
    // state
    float cash, units, invested, tp_price;
    int since, nper, last_dip;
    BtAccum acc;

    __device__ void load(const float* __restrict__ pr, float initial_equity)
    {
#pragma clang fp contract(off)
        period = max((int)pr[0], 1);
        base = pr[1] * initial_equity;
        four_base = 4.0f * base;
        dipk = 1.0f - pr[2];
        dip_mult = pr[3];
        cooldown = (int)pr[4];
        tpk = 1.0f + pr[5];
        va = pr[6] > 0.5f;
        cash = initial_equity;
        units = invested = tp_price = 0.f;
        since = nper = 0;
        last_dip = DC_NEVER;
        acc.init(initial_equity);
    }

    // Candle t, marked to market. `c` is the candle's {close, high,
    // rmax120, -} and must be bound to the LDS tile entry itself, not to a
    // register copy: the lane then reads close and rmax120 up front and
    // high only once it holds units, as the loop did before it was a
    // function. From a copy the compiler merges the two take-profit tests
    // into one mask and the metrics kernel is no longer the same kernel.
    template <class Rec>
    __device__ void step(int t, const float4& c, Rec& rec)
    {
#pragma clang fp contract(off)
        const float close = c.x, high = c.y, rmax = c.z;
        const float omf = 1.0f - BT_FEE;
        // --- 1. take profit ----------------------------------------------
        if (units > 0.0f && high >= tp_price) {
            const float proceeds = units * tp_price * omf;
            cash += proceeds;
            acc.trade(proceeds - invested);
            rec.take_profit(t, tp_price, units, proceeds,
                            proceeds - invested);
            units = 0.0f;
            invested = 0.0f;
            since = 0;
            nper = 0;
        } else {
            // --- 2. scheduled / dip buy ----------------------------------
            bool sched = false;
            if (++since == period) { since = 0; ++nper; sched = true; }
            const bool dip = (close < rmax * dipk) &&
                             (t - last_dip >= cooldown);
            if (sched || dip) {
                float usd = base;
                if (sched && va)
                    usd = fminf(fmaxf(base * (float)nper - units * close,
                                      0.0f), four_base);
                if (dip) { usd = usd * dip_mult; last_dip = t; }
                usd = fminf(usd, cash);
                if (usd > 0.0f) {
                    cash -= usd;
                    const float du = usd * omf / close;
                    units += du;
                    invested += usd;
                    tp_price = invested / units * tpk;
                    rec.buy(t, sched, dip, close, du, usd, units);
                }
            }
        }
        // --- 3. mark to market -------------------------------------------
        acc.mark(cash + units * close);
    }
};

// Stage tile [t0, t0 + BT_TILE) of one symbol for the lane loop:
// tile[tt] = {close, high, rmax120, -}, rmax120 cooperatively from the
// close halo, one thread per tile candle. Ends with a barrier.
// backtest_dca_kernel keeps these same lines in its own body: called
// from here the compiler unrolls the rmax120 loop another way and that
// kernel takes 52 VGPRs instead of its 50.
__device__ __forceinline__ void dca_stage_tile(
    const float4* __restrict__ sym_candles, int t0, int T, float* chist,
    float* shigh, float4* tile)
{
    const int tid = threadIdx.x;
    const int tend = min(BT_TILE, T - t0);
    __syncthreads();
    // stage [t0 - HALO, t0 + TILE); -inf left of t=0 (max identity)
    for (int i = tid; i < DC_SPAN; i += BT_BLOCK) {
        const int t = t0 - DC_HALO + i;
        float cl = -INFINITY, hi = 0.0f;
        if (t >= 0 && t < T) {
            const float4 c = sym_candles[t];
            cl = c.x;
            hi = c.y;
        }
        chist[i] = cl;
        if (i >= DC_HALO) shigh[i - DC_HALO] = hi;
    }
    __syncthreads();
    // cooperative shared series: one thread per tile candle
    if (tid < tend) {
        const int base_i = tid + DC_HALO;
        const int L = min(t0 + tid + 1, DC_LOOKBACK);
        float m = -INFINITY;
        for (int j = 0; j < L; ++j) m = fmaxf(m, chist[base_i - j]);
        tile[tid] = make_float4(chist[base_i], shigh[tid], m, 0.0f);
    }
    __syncthreads();
}

}  // namespace
