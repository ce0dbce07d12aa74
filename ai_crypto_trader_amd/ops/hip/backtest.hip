// GPU backtest engine — the headline kernel.
//
// Replaces the reference's per-candle Python loop
// (backtesting/strategy_tester.py:190-300, services/strategy_evaluation.py:777-878)
// with CDNA4 lanes marching candles:
//   - a block = 256 lanes; each lane simulates one param-set of one
//     symbol (96 VGPR, 5 waves/SIMD). A two-param-sets-per-lane variant
//     (two independent dependency chains/lane, 148 VGPR, 3 waves/SIMD)
//     was tried and removed: measured 10% SLOWER — 290 vs 323 G candles/s
//     at pop=1024 x 64 sym x 16 segments: wave-level latency hiding beats
//     in-lane ILP here because both chains stall on the same LDS
//     broadcast + f64 sequence.
//   - candle tiles staged in LDS with a MAX_WIN-candle HALO: close history
//     is shared by every lane of the block, so the Bollinger "ring buffer"
//     is just a broadcast read of close[t-W] from the halo tile — no
//     per-lane LDS state at all (v1 used 32 KB/block of per-lane rings and
//     was LDS-occupancy-bound at 4 waves/SIMD)
//   - EMA/MACD/Wilder-RSI are O(1) register recurrences per candle
//   - the position state machine (SL/TP/trailing/vote exits — semantics of
//     trade_executor_service.py:55-399 + binance_ml_strategy.py:489-543)
//     matches backtesting/engine_cpu.py bit-for-bit (fp-contract off, same
//     operation order, f64 Bollinger sums both sides).
//
// The indicator/vote step, tile staging and shared-series precompute are
// bt_vote.hpp (shared with backtest_tp.hip); the metrics accumulator and
// the block map are bt_common.hpp (shared with every backtest kernel).
//
// Grid: nsym * ceil(P/256) blocks, XCD-affine map keeps the blocks of one
// symbol on one XCD so their shared candle stream stays in that XCD's L2.

#include "bt_vote.hpp"

namespace {

// one strategy's full simulation state: indicators + position + metrics
struct BtState {
    VoteState v;
    float size_pct, sl_pct, tp_pct, trail_pct, trail_act;
    float cash, units;
    bool in_pos;
    float entry_cost, entry_price;
    float stop, tp, peak;
    BtAccum acc;

    __device__ void load(const float* __restrict__ pr, float initial_equity)
    {
        v.load(pr);
        size_pct = pr[12]; sl_pct = pr[13]; tp_pct = pr[14];
        trail_pct = pr[15]; trail_act = pr[16];
        cash = initial_equity; units = 0.f;
        in_pos = false;
        entry_cost = entry_price = stop = tp = peak = 0.f;
        acc.init(initial_equity);
    }

    template <bool SKIP_BB>
    __device__ void step(int t, float close, float high, float low,
                         float oldc, float change, float4 sv)
    {
#pragma clang fp contract(off)           // match the numpy f32 reference
        // --- 1+2. indicators, votes ----------------------------------
        const int net = v.template step<SKIP_BB>(
            t, close, change, oldc, (double)close * (double)close,
            (double)oldc * (double)oldc, sv);

        // --- 3. position management ----------------------------------
        if (in_pos) {
            peak = fmaxf(peak, high);
            bool trail_on = (trail_pct > 0.0f) &&
                            (peak >= entry_price * (1.0f + trail_act));
            if (trail_on)
                stop = fmaxf(stop, peak * (1.0f - trail_pct));
            bool hit_sl = low <= stop;
            bool hit_tp = !hit_sl && high >= tp;
            bool hit_sig = !hit_sl && !hit_tp && net <= -v.exit_v;
            if (hit_sl || hit_tp || hit_sig) {
                float exit_price = hit_sl ? stop : (hit_tp ? tp : close);
                float proceeds = units * exit_price * (1.0f - BT_FEE);
                cash += proceeds;
                acc.trade(proceeds - entry_cost);
                units = 0.0f;
                in_pos = false;
            }
        } else if (t >= BT_WARMUP && net >= v.entry_v) {
            float cost = fminf(size_pct * acc.equity, cash);
            units = cost * (1.0f - BT_FEE) / close;
            cash -= cost;
            entry_cost = cost;
            entry_price = close;
            stop = close * (1.0f - sl_pct);
            tp = close * (1.0f + tp_pct);
            peak = close;
            in_pos = true;
        }

        // --- 4. mark to market ---------------------------------------
        // flat lanes: new_eq == cash == equity exactly, so r == 0 and
        // every accumulator is unchanged — skipping is bit-identical
        // to engine_cpu.py (which computes r = cash/cash - 1 = 0)
        if (units != 0.0f || cash != acc.equity)
            acc.mark(cash + units * close);
    }
};

template <bool HAS_RESNAP>
// second arg: min resident blocks/CU — pins the allocation at <=102
// VGPR so 5 waves/SIMD stay resident (the resnap addition had silently
// inflated the allocation to 160 VGPR = 3 waves/SIMD, a 20% headline
// regression; measured: occupancy beats spill-free codegen here)
__global__ void __launch_bounds__(BT_BLOCK, 5) backtest_kernel(
    const float* __restrict__ candles,   // (nsym, T, 4)
    const float* __restrict__ pop,       // (P, NPARAM)
    float* __restrict__ metrics,         // (P, nsym, NMETRIC)
    int nsym, int T, int P, int chunks_per_sym, float initial_equity)
{
#pragma clang fp contract(off)           // match the numpy f32 reference
    __shared__ float chist[BT_SPAN];     // close history incl. halo
    __shared__ float hl[BT_SPAN][2];     // high, low
    __shared__ float4 sh_vote[BT_TILE];  // bt_shared_votes() per candle

    int sym, chunk;
    bt_block_map(blockIdx.x, nsym, chunks_per_sym, sym, chunk);
    const int tid = threadIdx.x;
    const int p = chunk * BT_BLOCK + tid;
    const bool act = p < P;

    BtState st;
    st.load(pop + (long)(act ? p : 0) * BT_NPARAM, initial_equity);

    float prev_close = 0.f;
    const float4* sym_candles =
        reinterpret_cast<const float4*>(candles + (long)sym * T * 4);

    for (int t0 = 0; t0 < T; t0 += BT_TILE) {
        bt_stage_tile(sym_candles, t0, T, chist, hl, nullptr);
        const int tend = min(BT_TILE, T - t0);
        // BB resnap at RESNAP-aligned tiles (engine_cpu.py lockstep):
        // window closes for candle t0 are chist[BT_HALO - j], j < bb_w.
        const bool resnap_tile = HAS_RESNAP && (t0 > 0) &&
                                 ((t0 & (BT_RESNAP - 1)) == 0);
        if (resnap_tile) st.v.resnap(&chist[BT_HALO]);
        bt_shared_votes(t0, tend, chist, hl, sh_vote);
        __syncthreads();
        int tt0 = 0;
        if (resnap_tile) {
            // peeled resnap candle: BB increment skipped (template
            // flag -> zero cost in the steady-state loop below)
            const float close = chist[BT_HALO];
            st.template step<true>(t0, close, hl[BT_HALO][0],
                                   hl[BT_HALO][1],
                                   chist[BT_HALO - st.v.bb_w],
                                   close - prev_close, sh_vote[0]);
            prev_close = close;
            tt0 = 1;
        }
        for (int tt = tt0; tt < tend; ++tt) {
            const int t = t0 + tt;
            const float close = chist[tt + BT_HALO];
            const float high = hl[tt + BT_HALO][0];
            const float low = hl[tt + BT_HALO][1];
            const float change = (t == 0) ? 0.0f : close - prev_close;
            const float4 sv = sh_vote[tt];   // b128 broadcast
            st.template step<false>(t, close, high, low,
                                    chist[tt + BT_HALO - st.v.bb_w],
                                    change, sv);
            prev_close = close;
        }
    }

    if (act)
        st.acc.finalize(metrics + ((long)p * nsym + sym) * BT_NMETRIC, T);
}

}  // namespace

extern "C" void launch_backtest(const float* candles, const float* pop,
                                float* metrics, int nsym, int T, int P,
                                float initial_equity, hipStream_t stream) {
    // histories short enough never to cross a RESNAP boundary run the
    // resnap-free instantiation: identical codegen (96 VGPR, 5 waves/
    // SIMD) to a kernel without the feature — the seg-64 headline path
    const int chunks = (P + BT_BLOCK - 1) / BT_BLOCK;
    auto k = T > BT_RESNAP ? backtest_kernel<true> : backtest_kernel<false>;
    hipLaunchKernelGGL(k, dim3(nsym * chunks), dim3(BT_BLOCK), 0, stream,
                       candles, pop, metrics, nsym, T, P, chunks,
                       initial_equity);
}
