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
//   - candle tiles staged in LDS with a 64-candle HALO: close history is
//     shared by every lane of the block, so the Bollinger "ring buffer"
//     is just a read of close[t-W] from the halo tile — no per-lane LDS
//     state at all (v1 used 32 KB/block of per-lane rings and was
//     LDS-occupancy-bound at 4 waves/SIMD)
//   - Bollinger {mean, std} depend on the strategy only through its
//     window length, an integer in [2, 32], so a block computes them once
//     per candle and window instead of once per lane (up to 8x redundant
//     f64 + sqrt before): per 32-candle sub-tile, 31 lanes of wave 0 (one
//     per window) march the f64 rolling sums into an LDS table
//     [candle][window], then all 256 lanes convert its slots to
//     {mean, std} in place, and every lane reads its window's slot
//   - everything else a lane needs of a candle is one 32-byte LDS record,
//     written by one thread per candle: {close, high, low, change} and
//     the four parameter values at which the candle's stochastic and
//     Williams votes flip (bt_vote_flip) — two b128 broadcasts off one
//     address; the close-to-close change and the products threshold *
//     range are computed once per block, not once per lane, and a lane
//     compares its own four parameters. The trend vote rides in the
//     third dword of the lane's Bollinger slot (one b96 read)
//   - EMA/MACD/Wilder-RSI are O(1) register recurrences per candle; the
//     EMAs are seeded with close[0], so no candle tests t == 0
//   - the first WARMUP = 4 sub-tiles of a history run the recurrences
//     only (no table conversion, no votes, no position machine), so the
//     main lane loop carries no t >= WARMUP test
//   - the lane loop is the whole cost (15625 candles x ~176 instructions
//     a wave), so it holds no instruction the result does not need:
//     bt_max / bt_min instead of canonicalising fmaxf / fminf, the
//     trailing trigger computed at entry, thread-indexed LDS addresses
//     rebuilt per tile instead of living through it, and the drawdown
//     divide behind a division-free test that skips it, bit for bit, on
//     the candles where it cannot raise max_dd (BtAccum::mark: a wave
//     needs it on under half of its candles). 31744 B of LDS and 96 VGPR
//     per lane keep five blocks on a CU — a 1 KB trend array on top,
//     32768 B, measured 7% slower, as if only four fit — and a dword of
//     scratch is reloaded once per tile and one per sub-tile, none in the
//     lane loop (see BtState::load)
//   - the position state machine (SL/TP/trailing/vote exits — semantics of
//     trade_executor_service.py:55-399 + binance_ml_strategy.py:489-543)
//     matches backtesting/engine_cpu.py bit-for-bit (fp-contract off, same
//     operation order, f64 Bollinger sums both sides).
//
// The indicator/vote step, tile staging and shared-series precompute are
// bt_vote.hpp (shared with backtest_tp.hip); the position machine is
// bt_position.hpp (shared with backtest_ledger.hip); the metrics
// accumulator and the block map are bt_common.hpp (shared with every
// backtest kernel).
//
// Grid: nsym * ceil(P/256) blocks, XCD-affine map keeps the blocks of one
// symbol on one XCD so their shared candle stream stays in that XCD's L2.

#include "bt_position.hpp"

namespace {

// one strategy's full simulation state: indicators + votes (bt_vote.hpp)
// and position + metrics (bt_position.hpp)
struct BtState {
    VoteState v;
    BtPosition pos;

    __device__ void load(const float* __restrict__ pr, float initial_equity)
    {
        v.load(pr);
        pos.load(pr, initial_equity);
        // Keep the two Williams thresholds in registers: left to itself
        // the compiler recomputes stoch_* - 100 in every candle to save
        // two VGPRs. Holding them costs one dword of scratch, reloaded
        // once per tile, and measured 1.9% faster than the spill-free
        // build (profiles/backtest_seg64_lane_loop.json).
        asm volatile("" : "+v"(v.will_os), "+v"(v.will_ob));
    }

    // One candle at t >= WARMUP. `c` = {close, high, low, change} and `sv`
    // = the four vote thresholds, the candle's LDS record; `trend` = its
    // trend vote; `ms` = {mean, std} of this lane's Bollinger window at
    // candle t. The EMAs were seeded.
    __device__ void step(int t, float4 c, float2 ms, float4 sv, int trend)
    {
#pragma clang fp contract(off)           // match the numpy f32 reference
        // --- 1+2. indicators, votes ----------------------------------
        const int net = v.count<false, true>(
            t, c.x, v.recur<true>(t, c.x, c.w), ms, sv, trend);
        // --- 3+4. position, mark to market; this kernel keeps only the
        // metrics, so what the candle did (the event) is dropped
        pos.step<false>(t, net, v.entry_v, v.exit_v, c.x, c.y, c.z);
    }

    // One candle at t < WARMUP: no vote is taken, so nothing can be
    // entered, the lane stays flat and its mark to market is the no-op
    // BtPosition::step skips — only the recurrences advance.
    __device__ void warm(int t, float4 c)
    {
        v.recur<true>(t, c.x, c.w);
    }
};

// Candles per fill of the Bollinger table. 32 candles x 32 window slots
// x 16 B = 16 KB. With the staging (320 x (4 + 8 + 8) B = 6400 B), the
// candle records (256 x 32 B = 8 KB) and the scan state (3 x 32 x 8 B)
// that is 31744 B per block, so the five blocks per CU that the VGPR
// budget allows also fit its 160 KB of LDS.
#define BT_BBSUB 32
static_assert(BT_TILE % BT_BBSUB == 0, "sub-tiles must tile the tile");
static_assert(BT_WARMUP % BT_BBSUB == 0 && BT_WARMUP <= BT_TILE,
              "the warm-up is whole sub-tiles of the first tile");
static_assert(BT_BLOCK % BT_MAXWIN == 0 && BT_BBSUB <= BT_BLOCK &&
                  (BT_MAXWIN & (BT_MAXWIN - 1)) == 0,
              "a lane converts slots of one window only");
// The table leaves out the early-window divisor (t + 1 < w): it only
// exists below MAX_WIN, and no vote is taken before WARMUP, so those
// entries are never consumed — the sums themselves advance from t = 0.
static_assert(BT_MAXWIN <= BT_WARMUP, "early-window entries are unused");

// a table slot holds either the f64 sums {sum, sum2} of (candle, window)
// or, once converted, {mean, std} in its first 8 bytes
__device__ inline float4 bt_pack_sums(double a, double b)
{
    return make_float4(__int_as_float(__double2loint(a)),
                       __int_as_float(__double2hiint(a)),
                       __int_as_float(__double2loint(b)),
                       __int_as_float(__double2hiint(b)));
}

__device__ inline double bt_unpack_sum(float lo, float hi)
{
    return __hiloint2double(__float_as_int(hi), __float_as_int(lo));
}

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
    __shared__ double csq[BT_SPAN];      // (double)close^2, same span
    __shared__ float hl[BT_SPAN][2];     // high, low
    // one record per candle: {close, high, low, change}, then the shared
    // votes (bt_shared_votes<true>) — two b128 broadcasts off one address
    __shared__ float4 rec[BT_TILE][2];
    // The record's ninth dword, the trend vote, has no LDS of its own
    // (1 KB more makes five blocks a CU's whole 160 KB, and measured 7%
    // slower, see profiles/backtest_seg64_exact_cuts.json): between
    // bt_shared_votes and the next staging nothing reads hl, so it rests
    // there until phase B moves it into the candle's table slots, where a
    // lane's {mean, std} read picks it up.
    int* trend = reinterpret_cast<int*>(&hl[0][0]);
    static_assert(sizeof(int) * BT_TILE <= sizeof(float) * 2 * BT_SPAN,
                  "the trend votes fit the dead high/low staging");
    // Bollinger table [sub-tile candle][window - 2]; slot 31 is padding
    __shared__ float4 bbtab[BT_BBSUB * BT_MAXWIN];
    // per window slot: the rolling sums between sub-tiles, and 1/w
    __shared__ double sh_sum[BT_MAXWIN], sh_sum2[BT_MAXWIN];
    __shared__ double sh_invw[BT_MAXWIN];

    int sym, chunk;
    bt_block_map(blockIdx.x, nsym, chunks_per_sym, sym, chunk);
    const int tid = threadIdx.x;
    const int p = chunk * BT_BLOCK + tid;
    const bool act = p < P;

    BtState st;
    st.load(pop + (long)(act ? p : 0) * BT_NPARAM, initial_equity);
    const float4* my_bb = bbtab + (st.v.bb_w - 2);

    // The scan lanes: lane j < 31 of wave 0 owns window j + 2, whatever
    // strategies the block holds, active or not. Its sums live in LDS
    // between sub-tiles, so no lane carries f64 state through the candle
    // loop.
    if (tid < BT_MAXWIN) {
        BollState b;
        b.init(tid + 2);
        sh_sum[tid] = b.sum;
        sh_sum2[tid] = b.sum2;
        sh_invw[tid] = b.inv_w;
    }
    if (tid < BT_BBSUB)                  // the padding slots: defined bits
        bbtab[tid * BT_MAXWIN + BT_MAXWIN - 1] =
            make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    const float4* sym_candles =
        reinterpret_cast<const float4*>(candles + (long)sym * T * 4);
    // Seed the EMAs with this symbol's first close instead of selecting on
    // t == 0 in every candle: candle 0 then computes x + a * (x - x), which
    // is x exactly for any finite a, and the alphas 2 / (period + 1) of
    // parameters within PARAM_BOUNDS lie in (0, 1].
    if (T > 0) st.v.ema_f = st.v.ema_s = sym_candles[0].x;

    for (int t0 = 0; t0 < T; t0 += BT_TILE) {
        // A copy of tid the compiler cannot see through. The staging, the
        // scan and the conversion address LDS by thread; derived from tid
        // itself, a dozen such addresses were hoisted to kernel entry and
        // then spilled around the lane loop. From this copy they are
        // recomputed once per tile.
        int ltid = tid;
        asm volatile("" : "+v"(ltid));
        const int scan_w = ltid + 2;
        const bool is_scan = scan_w <= BT_MAXWIN;
        bt_stage_tile(sym_candles, t0, T, chist, hl, csq, ltid);
        const int tend = min(BT_TILE, T - t0);
        // BB resnap at RESNAP-aligned tiles (engine_cpu.py lockstep):
        // window closes for candle t0 are chist[BT_HALO - j], j < w; the
        // resnap candle itself then takes no increment.
        const bool resnap_tile = HAS_RESNAP && (t0 > 0) &&
                                 ((t0 & (BT_RESNAP - 1)) == 0);
        if (resnap_tile && is_scan) {
            BollState b;
            b.resnap(scan_w, &chist[BT_HALO]);
            sh_sum[ltid] = b.sum;
            sh_sum2[ltid] = b.sum2;
        }
        const int my_trend =
            bt_shared_votes<true>(t0, tend, chist, hl, &rec[0][0], ltid);
        __syncthreads();                 // every thread is done with hl
        trend[ltid] = my_trend;
        for (int s0 = 0; s0 < tend; s0 += BT_BBSUB) {
            const int send = min(s0 + BT_BBSUB, tend);
            // a warm-up sub-tile lies below WARMUP as a whole
            const bool warm = t0 + s0 < BT_WARMUP;
            // the previous sub-tile's readers are done with the table
            // (s0 == 0: bt_stage_tile's barriers already say so)
            if (s0 > 0) __syncthreads();
            // phase A, scan lanes only: the sums are an inexact, order-
            // dependent chain, so they march sequentially from candle 0 —
            // but nothing else does; a slot gets the sums as of its candle
            if (is_scan) {
                BollState b;
                b.sum = sh_sum[ltid];
                b.sum2 = sh_sum2[ltid];
#pragma unroll 4
                for (int tt = s0; tt < send; ++tt) {
                    const int i = tt + BT_HALO;
                    if (!(resnap_tile && tt == 0))
                        b.advance(chist[i], chist[i - scan_w], csq[i],
                                  csq[i - scan_w]);
                    bbtab[(tt - s0) * BT_MAXWIN + ltid] =
                        bt_pack_sums(b.sum, b.sum2);
                }
                sh_sum[ltid] = b.sum;
                sh_sum2[ltid] = b.sum2;
            }
            __syncthreads();             // sums (and the records) visible
            if (warm) {
                // no vote reads the table before WARMUP: the recurrences
                // advance, phase B and the position machine are skipped
                for (int tt = s0; tt < send; ++tt)
                    st.warm(t0 + tt, rec[tt][0]);
                continue;
            }
            // phase B, the whole block: sums -> {mean, std} in place, the
            // f64 multiplies and the sqrt spread over all lanes. A lane's
            // slots all belong to one window (BT_BLOCK % BT_MAXWIN == 0).
            {
                BollState b;
                b.inv_w = sh_invw[ltid & (BT_MAXWIN - 1)];
                for (int e = ltid; e < (send - s0) * BT_MAXWIN;
                     e += BT_BLOCK) {
                    const float4 v = bbtab[e];
                    b.sum = bt_unpack_sum(v.x, v.y);
                    b.sum2 = bt_unpack_sum(v.z, v.w);
                    const float2 ms = b.stats<false>(0, 0);
                    bbtab[e].x = ms.x;
                    bbtab[e].y = ms.y;
                    bbtab[e].z =
                        __int_as_float(trend[s0 + e / BT_MAXWIN]);
                }
            }
            __syncthreads();             // table visible
            for (int tt = s0; tt < send; ++tt) {
                // b96 per lane, {mean, std, trend}: equal windows
                // broadcast, distinct windows sit 16 B apart
                const float4* e = &my_bb[(tt - s0) * BT_MAXWIN];
                st.step(t0 + tt, rec[tt][0], make_float2(e->x, e->y),
                        rec[tt][1], __float_as_int(e->z));
            }
        }
    }

    // p again from an opaque tid, as above: otherwise it is spilled at
    // entry and reloaded here
    int otid = tid;
    asm volatile("" : "+v"(otid));
    const int po = chunk * BT_BLOCK + otid;
    if (po < P)
        st.pos.acc.finalize(metrics + ((long)po * nsym + sym) * BT_NMETRIC,
                            T);
}

}  // namespace

extern "C" void launch_backtest(const float* candles, const float* pop,
                                float* metrics, int nsym, int T, int P,
                                float initial_equity, hipStream_t stream) {
    // histories short enough never to cross a RESNAP boundary run the
    // resnap-free instantiation: the same codegen as a kernel without
    // the feature — the seg-64 headline path
    const int chunks = (P + BT_BLOCK - 1) / BT_BLOCK;
    auto k = T > BT_RESNAP ? backtest_kernel<true> : backtest_kernel<false>;
    hipLaunchKernelGGL(k, dim3(nsym * chunks), dim3(BT_BLOCK), 0, stream,
                       candles, pop, metrics, nsym, T, P, chunks,
                       initial_equity);
}
