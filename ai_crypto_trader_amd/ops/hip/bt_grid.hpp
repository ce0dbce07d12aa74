// The grid family's per-lane state machine (backtesting/strategy_grid.py is
// the contract), shared by backtest_grid.hip (metrics only) and
// backtest_fills.hip (metrics plus one record per fill). Why the level
// table is a [level][lane] LDS array with a register cursor on top, and
// how the sell / buy masks are built: backtest_grid.hip's header.
//
// Recorder: build() and step() take a compile-time recorder and call
// rec.fill() once per fill, in the record order of backtesting/fills.py.
// What the recorder needs to remember is the recorder type's own state,
// not the lane's. GridNoFills has an empty inline hook: its arguments are
// values the state machine computes anyway or dead conversions of them,
// so backtest_grid_kernel compiles to what it was before the hook
// existed.
#pragma once

#include "bt_common.hpp"

#define GR_NPARAM 5
#define GR_MAXHALF 16            // == strategy_grid.py MAX_HALF
#define GR_NLEV (2 * GR_MAXHALF + 1)

// == fills.py FILL_KINDS[0..3]
#define GR_FILL_BUY 0
#define GR_FILL_SELL 1
#define GR_FILL_BUILD 2
#define GR_FILL_BREAKOUT 3

namespace {

struct GridNoFills {
    __device__ __forceinline__ void fill(int, int, int, float, float, float,
                                         float, float) {}
};

struct GridLane {
    // params
    int H, twoH;
    uint32_t slotmask;
    float s, cf, up_k, dn_k;
    bool geo;
    // grid state
    uint32_t filled, initial;
    float b, bomf, u0;
    float sell_px, buy_px, up_thr, dn_thr;
    float cash;
    double units_total;
    BtAccum acc;

    __device__ void load(const float* __restrict__ pr, float initial_equity)
    {
#pragma clang fp contract(off)
        H = min(max((int)pr[0], 1), GR_MAXHALF);
        twoH = 2 * H;
        slotmask = (twoH >= 32) ? 0xffffffffu : ((1u << twoH) - 1u);
        s = pr[1];
        geo = pr[2] > 0.5f;
        cf = pr[3];
        up_k = 1.0f + pr[4];
        dn_k = 1.0f - pr[4];
        filled = initial = 0u;
        b = bomf = u0 = 0.f;
        sell_px = buy_px = up_thr = dn_thr = 0.f;
        cash = initial_equity;
        units_total = 0.0;
        acc.init(initial_equity);
    }

    // units held by filled slot k
    __device__ float slot_units(const float (*lev)[BT_BLOCK], int tid,
                                int k) const
    {
#pragma clang fp contract(off)
        return ((initial >> k) & 1u) ? u0 : bomf / lev[k][tid];
    }

    // reload the two cursor levels from the table
    __device__ void refresh_px(const float (*lev)[BT_BLOCK], int tid)
    {
        const uint32_t empt = ~filled & slotmask;
        sell_px = filled ? lev[__ffs((int)filled)][tid] : INFINITY;
        buy_px = empt ? lev[31 - __clz((int)empt)][tid] : -INFINITY;
    }

    template <class Rec>
    __device__ void build(float (*lev)[BT_BLOCK], int tid, int t,
                          float close, Rec& rec)
    {
#pragma clang fp contract(off)
        const float omf = 1.0f - BT_FEE;
        b = cf * cash / (float)twoH;
        bomf = b * omf;
        u0 = bomf / close;
        cash = cash - (float)H * b;
        units_total = (double)H * (double)u0;
        lev[H][tid] = close;
        float up = close, dn = close;
        if (geo) {
            const float r = 1.0f + s;
            for (int j = 1; j <= H; ++j) {
                up = up * r;
                dn = dn / r;
                lev[H + j][tid] = up;
                lev[H - j][tid] = dn;
            }
        } else {
            const float step = close * s;
            for (int j = 1; j <= H; ++j) {
                up = close + (float)j * step;
                dn = close - (float)j * step;
                lev[H + j][tid] = up;
                lev[H - j][tid] = dn;
            }
        }
        // the H market fills, ascending k from H; the f32 product
        // (float)H * u0 is the correctly rounded exact product, i.e.
        // (float)units_total
        for (int j = 1; j <= H; ++j)
            rec.fill(t, GR_FILL_BUILD, H + j - 1, close, u0, -b, 0.0f,
                     (float)j * u0);
        filled = slotmask & ~((1u << H) - 1u);
        initial = filled;
        up_thr = up * up_k;
        dn_thr = dn * dn_k;
        refresh_px(lev, tid);
    }

    template <class Rec>
    __device__ void step(float (*lev)[BT_BLOCK], int tid, int t, float close,
                         float high, float low, Rec& rec)
    {
#pragma clang fp contract(off)
        const float omf = 1.0f - BT_FEE;
        const uint32_t f0 = filled;          // pre-candle fill state
        bool touched = false;
        // --- 1. sells, ascending k ---------------------------------------
        if (high >= sell_px) {
            uint32_t m = f0;
            while (m) {
                const int k = __ffs((int)m) - 1;
                const float lk1 = lev[k + 1][tid];
                if (!(high >= lk1)) break;
                const float uk = slot_units(lev, tid, k);
                const float proceeds = uk * lk1 * omf;
                cash += proceeds;
                units_total -= (double)uk;
                acc.trade(proceeds - b);
                filled &= ~(1u << k);
                m &= m - 1u;
                rec.fill(t, GR_FILL_SELL, k, lk1, uk, proceeds, proceeds - b,
                         (float)units_total);
            }
            touched = true;
        }
        // --- 2. buys, descending k ---------------------------------------
        if (low <= buy_px) {
            uint32_t m = ~f0 & slotmask;
            while (m) {
                const int k = 31 - __clz((int)m);
                const float lk = lev[k][tid];
                if (!(low <= lk) || !(cash >= b)) break;
                cash -= b;
                const float uk = bomf / lk;
                units_total += (double)uk;
                filled |= 1u << k;
                initial &= ~(1u << k);
                m &= ~(1u << k);
                rec.fill(t, GR_FILL_BUY, k, lk, uk, -b, 0.0f,
                         (float)units_total);
            }
            touched = true;
        }
        // --- 3. breakout: liquidate at close, rebuild --------------------
        if (close > up_thr || close < dn_thr) {
            uint32_t m = filled;
            while (m) {
                const int k = __ffs((int)m) - 1;
                const float uk = slot_units(lev, tid, k);
                const float proceeds = uk * close * omf;
                cash += proceeds;
                acc.trade(proceeds - b);
                m &= m - 1u;
                // units_total is not touched here (build() overwrites it)
                rec.fill(t, GR_FILL_BREAKOUT, k, close, uk, proceeds,
                         proceeds - b, (float)units_total);
            }
            build(lev, tid, t, close, rec);
        } else if (touched) {
            refresh_px(lev, tid);
        }
    }
};

}  // namespace
