// The vote family's position machine (strategy.py step 3 + 4), once, for
// the kernels that march it per candle behind their own vote count:
// backtest.hip (headline, metrics only) and backtest_ledger.hip (trade
// records + equity samples). SL/TP/trailing/vote exits — semantics of
// trade_executor_service.py:55-399 + binance_ml_strategy.py:489-543 —
// matching backtesting/engine_cpu.py bit for bit (fp-contract off, same
// operation order). backtest_tp.hip's TradeState is the branchless form
// of the same contract for a different latency regime; see its comment.
#pragma once

#include "bt_vote.hpp"

// what one candle did to the position: nothing, an entry, or an exit for
// one of StrategyTester.Trade.reason's three causes (ledger.py REASONS;
// the ledger splits a stop exit further into stop_loss / trailing_stop)
#define BT_EV_NONE 0
#define BT_EV_STOP 1
#define BT_EV_TP 2
#define BT_EV_SIGNAL 3
#define BT_EV_ENTRY (-1)

struct BtEvent {
    int kind;
    float price;      // exit fill: stop, tp or close (exits only)
    float pnl;        // the value handed to BtAccum::trade (exits only)
};

// position + metrics state of one strategy
struct BtPosition {
    float size_pct, sl_pct, tp_pct;
    float trail_m, act_m;     // 1 - trailing_stop_pct, 1 + trailing_act_pct
    bool trail_en;            // trailing_stop_pct > 0
    float cash, units;
    bool in_pos;
    float entry_cost, entry_price;
    float trail_trig;         // entry_price * act_m: constant while in
    float stop, tp, peak;
    BtAccum acc;

    __device__ void load(const float* __restrict__ pr, float initial_equity)
    {
#pragma clang fp contract(off)
        size_pct = pr[12]; sl_pct = pr[13]; tp_pct = pr[14];
        trail_m = 1.0f - pr[15]; act_m = 1.0f + pr[16];
        trail_en = pr[15] > 0.0f;
        cash = initial_equity; units = 0.f;
        in_pos = false;
        entry_cost = entry_price = trail_trig = stop = tp = peak = 0.f;
        acc.init(initial_equity);
    }

    // One candle: `net` is the vote count, entry_v / exit_v the
    // strategy's thresholds. A caller that ignores the returned event
    // pays nothing for it. WARM_TEST = false is for a caller that only
    // comes here with t >= WARMUP.
    template <bool WARM_TEST = true>
    __device__ BtEvent step(int t, int net, int entry_v, int exit_v,
                            float close, float high, float low)
    {
#pragma clang fp contract(off)           // match the numpy f32 reference
        BtEvent ev = {BT_EV_NONE, 0.0f, 0.0f};
        // --- 3. position management ----------------------------------
        if (in_pos) {
            peak = bt_max(peak, high);
            bool trail_on = trail_en && (peak >= trail_trig);
            if (trail_on)
                stop = bt_max(stop, peak * trail_m);
            bool hit_sl = low <= stop;
            bool hit_tp = !hit_sl && high >= tp;
            bool hit_sig = !hit_sl && !hit_tp && net <= -exit_v;
            if (hit_sl || hit_tp || hit_sig) {
                float exit_price = hit_sl ? stop : (hit_tp ? tp : close);
                float proceeds = units * exit_price * (1.0f - BT_FEE);
                cash += proceeds;
                acc.trade(proceeds - entry_cost);
                ev.kind = hit_sl ? BT_EV_STOP
                                 : (hit_tp ? BT_EV_TP : BT_EV_SIGNAL);
                ev.price = exit_price;
                ev.pnl = proceeds - entry_cost;
                units = 0.0f;
                in_pos = false;
            }
        } else if ((!WARM_TEST || t >= BT_WARMUP) && net >= entry_v) {
            float cost = bt_min(size_pct * acc.equity, cash);
            units = cost * (1.0f - BT_FEE) / close;
            cash -= cost;
            entry_cost = cost;
            entry_price = close;
            trail_trig = close * act_m;
            stop = close * (1.0f - sl_pct);
            tp = close * (1.0f + tp_pct);
            peak = close;
            in_pos = true;
            ev.kind = BT_EV_ENTRY;
        }

        // --- 4. mark to market ---------------------------------------
        // flat lanes: new_eq == cash == equity exactly, so r == 0 and
        // every accumulator is unchanged — skipping is bit-identical
        // to engine_cpu.py (which computes r = cash/cash - 1 = 0)
        if (units != 0.0f || cash != acc.equity)
            acc.mark(cash + units * close);
        return ev;
    }
};
