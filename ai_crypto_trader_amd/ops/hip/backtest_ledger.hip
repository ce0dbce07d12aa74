// Trade ledger + equity curves of the vote backtest.
//
// backtest.hip returns ten aggregates per (strategy, symbol); this kernel
// runs the same simulation and also says which trades it made — the
// record the reference's backtester is built around
// (backtesting/strategy_tester.py:314-357: entry/exit time and price,
// quantity, pnl, exit_reason) — and samples the equity curve on the way.
// CPU twin: engine_cpu.run_backtest_cpu(record_trades=True); layout and
// field meanings: backtesting/ledger.py.
//
// One lane per (strategy, symbol), backtest.hip's block map and tile
// staging. It is meant for inspecting few strategies over many symbols
// and a long history, so:
//   - Bollinger sums are per lane (VoteState::step<>, the resnap candle
//     peeled as in bt_flags_kernel), not backtest.hip's block table: the
//     two are bit-identical by contract, and with a handful of strategies
//     per block the table's cooperation buys nothing;
//   - at small P the launch is one serial chain per lane and latency-
//     bound. That is accepted — what it replaces is a Python loop.
//
// Recorder: the pending record lives in registers (entry price and cost
// are the position machine's own, plus the entry candle and the units);
// the full 32-byte record is written once, at the exit, or at T for a
// position still open. Trade writes are rare and divergent, so they go
// lane-major (P, nsym, max_trades, 8). Equity samples are written every
// `stride` candles by all lanes at once, so they go time-major with the
// strategy index fastest, (nsym, n_samples, P), like bt_flags_kernel's
// bitmaps: a wave's stores coalesce. All offsets are 64-bit.

#include "bt_position.hpp"

#define BT_REASON_TRAIL 4      // == ledger.py REASONS[4]

namespace {

struct Ledger {
    float4* __restrict__ rec;      // this lane's max_trades x 2 float4
    float* __restrict__ eq;        // equity + sym * n_samples * P + p
    long eq_step;                  // P
    int max_trades, stride;
    bool act;
    int nrec;                      // positions opened and recorded so far
    int pend_t;                    // entry candle of the open position
    float pend_units;              // units bought there
    int cnt;                       // candles since the last equity sample

    // slot `nrec` gets the record if the lane has room for it: overflow
    // drops the newest records and still counts them
    __device__ void write(const BtPosition& pos, int exit_t, int reason,
                          float exit_price, float pnl)
    {
        if (act && nrec < max_trades) {
            rec[2 * (long)nrec] = make_float4(
                __int_as_float(pend_t), __int_as_float(exit_t),
                __int_as_float(reason), pos.entry_price);
            rec[2 * (long)nrec + 1] =
                make_float4(exit_price, pend_units, pos.entry_cost, pnl);
        }
        ++nrec;
    }

    // after BtPosition::step of candle t
    __device__ void candle(int t, const BtPosition& pos, BtEvent ev)
    {
#pragma clang fp contract(off)           // match the numpy f32 reference
        if (ev.kind == BT_EV_ENTRY) {
            pend_t = t;
            pend_units = pos.units;
        } else if (ev.kind != BT_EV_NONE) {
            int reason = ev.kind;
            // a stop that trailing raised above where the entry put it
            // (the same f32 product as BtPosition::step's entry)
            if (reason == BT_EV_STOP &&
                ev.price > pos.entry_price * (1.0f - pos.sl_pct))
                reason = BT_REASON_TRAIL;
            write(pos, t, reason, ev.price, ev.pnl);
        }
        if (++cnt == stride) {
            if (act) *eq = pos.acc.equity;
            eq += eq_step;
            cnt = 0;
        }
    }

    // after the last candle: the open position, the final equity sample
    __device__ void finish(const BtPosition& pos)
    {
        if (pos.in_pos) write(pos, -1, 0, 0.0f, 0.0f);
        if (cnt > 0 && act) *eq = pos.acc.equity;
    }
};

__global__ void __launch_bounds__(BT_BLOCK) backtest_ledger_kernel(
    const float* __restrict__ candles,   // (nsym, T, 4)
    const float* __restrict__ pop,       // (P, NPARAM)
    float* __restrict__ metrics,         // (P, nsym, NMETRIC)
    int* __restrict__ n_records,         // (P, nsym)
    float4* __restrict__ records,        // (P, nsym, max_trades, 2)
    float* __restrict__ equity,          // (nsym, n_samples, P)
    int nsym, int T, int P, int chunks_per_sym, int max_trades, int stride,
    int n_samples, float initial_equity)
{
#pragma clang fp contract(off)           // match the numpy f32 reference
    __shared__ float chist[BT_SPAN];     // close history incl. halo
    __shared__ double csq[BT_SPAN];      // (double)close^2, same span
    __shared__ float hl[BT_SPAN][2];     // high, low
    __shared__ float4 sh_vote[BT_TILE];  // bt_shared_votes() per candle

    int sym, chunk;
    bt_block_map(blockIdx.x, nsym, chunks_per_sym, sym, chunk);
    const int tid = threadIdx.x;
    const int p = chunk * BT_BLOCK + tid;
    const bool act = p < P;
    const long pc = act ? p : 0;         // idle lanes: in-bounds, no stores

    VoteState v;
    BtPosition pos;
    v.load(pop + pc * BT_NPARAM);
    pos.load(pop + pc * BT_NPARAM, initial_equity);

    const long lane = pc * nsym + sym;
    Ledger lg;
    lg.rec = records + lane * max_trades * 2;
    lg.eq = equity + (long)sym * n_samples * P + pc;
    lg.eq_step = P;
    lg.max_trades = max_trades;
    lg.stride = stride;
    lg.act = act;
    lg.nrec = 0;
    lg.pend_t = -1;
    lg.pend_units = 0.0f;
    lg.cnt = 0;

    float prev_close = 0.f;
    const float4* sym_candles =
        reinterpret_cast<const float4*>(candles + (long)sym * T * 4);

    for (int t0 = 0; t0 < T; t0 += BT_TILE) {
        bt_stage_tile(sym_candles, t0, T, chist, hl, csq);
        const int tend = min(BT_TILE, T - t0);
        bt_shared_votes(t0, tend, chist, hl, sh_vote);
        __syncthreads();

        // BB resnap at RESNAP-aligned tiles (engine_cpu.py lockstep), the
        // resnap candle peeled (compile-time SKIP_BB) as in
        // bt_flags_kernel
        int tt0 = 0;
        if ((t0 > 0) && ((t0 & (BT_RESNAP - 1)) == 0)) {
            v.resnap(&chist[BT_HALO]);
            const float close = chist[BT_HALO];
            const int net = v.step<true>(
                t0, close, close - prev_close, chist[BT_HALO - v.bb_w],
                csq[BT_HALO], csq[BT_HALO - v.bb_w], sh_vote[0]);
            lg.candle(t0, pos,
                      pos.step(t0, net, v.entry_v, v.exit_v, close,
                               hl[BT_HALO][0], hl[BT_HALO][1]));
            prev_close = close;
            tt0 = 1;
        }
        for (int tt = tt0; tt < tend; ++tt) {
            const int t = t0 + tt;
            const int i = tt + BT_HALO;
            const float close = chist[i];
            const float change = (t == 0) ? 0.0f : close - prev_close;
            const int net = v.step<false>(
                t, close, change, chist[i - v.bb_w], csq[i],
                csq[i - v.bb_w], sh_vote[tt]);
            lg.candle(t, pos,
                      pos.step(t, net, v.entry_v, v.exit_v, close,
                               hl[i][0], hl[i][1]));
            prev_close = close;
        }
    }

    lg.finish(pos);
    if (act) {
        n_records[lane] = lg.nrec;
        pos.acc.finalize(metrics + lane * BT_NMETRIC, T);
    }
}

}  // namespace

extern "C" void launch_backtest_ledger(
    const float* candles, const float* pop, float* metrics, int* n_records,
    float* records, float* equity, int nsym, int T, int P, int max_trades,
    int stride, int n_samples, float initial_equity, hipStream_t stream)
{
    const int chunks = (P + BT_BLOCK - 1) / BT_BLOCK;
    hipLaunchKernelGGL(backtest_ledger_kernel, dim3(nsym * chunks),
                       dim3(BT_BLOCK), 0, stream, candles, pop, metrics,
                       n_records, reinterpret_cast<float4*>(records),
                       equity, nsym, T, P, chunks, max_trades, stride,
                       n_samples, initial_equity);
}
