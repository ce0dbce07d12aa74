// Fill ledgers + equity curves of the grid and DCA families.
//
// backtest_grid.hip / backtest_dca.hip return ten aggregates per
// (strategy, symbol); these two kernels run the same state machines — the
// one copy of each, bt_grid.hpp's GridLane and bt_dca.hpp's DcaLane, here
// instantiated with a recorder that writes — and also say what each lane
// did: one 32-byte record per fill (which level bought or sold when, what
// a breakout liquidated, each DCA order and take-profit), the per-order
// events the reference's grid and DCA bots log, plus the sampled equity
// curve. CPU twins: engine_grid_cpu.run_grid_backtest_cpu /
// engine_dca_cpu.run_dca_backtest_cpu with record_fills=True; layout,
// field meanings and record order: backtesting/fills.py.
//
// Modelled on backtest_ledger.hip. One lane per (strategy, symbol), the
// family kernels' block map and tile staging (the grid keeps its
// [level][lane] LDS table). Meant for inspecting few strategies over many
// symbols and a long history: at small P a launch is one latency-bound
// serial chain per lane, and a grid lane can write thousands of divergent
// records. Both are accepted — what this replaces is a Python loop.
//
// A record is written whole, as two float4 stores, the moment the state
// machine fills, into the lane's own run of (P, nsym, max_fills, 8): slot
// `nrec` if act && nrec < max_fills, and nrec counts either way (overflow
// drops the newest and still counts them). Equity samples are written
// every `stride` candles by all lanes at once, so they go time-major with
// the strategy index fastest, (nsym, n_samples, P): a wave's stores
// coalesce. All offsets are 64-bit. Idle lanes of a partial block run
// lane 0's parameters in bounds and store nothing.
//
// Compiler resource report (hipcc -O3, gfx950, -Rpass-analysis=
// kernel-resource-usage):
//   backtest_grid_fills_kernel: 84 VGPR, 0 AGPR, 48 SGPR, 0 B scratch, no
//     spills, 37,888 B LDS/block, occupancy 4 waves/SIMD (LDS-limited,
//     like backtest_grid_kernel at 66 VGPR);
//   backtest_dca_fills_kernel: 62 VGPR, 0 AGPR, 46 SGPR, 0 B scratch, no
//     spills, 6,656 B LDS/block, occupancy 8 waves/SIMD.
// Measured time against the numpy twins: docs/KERNELS.md "Family fill
// ledgers".

#include "bt_dca.hpp"
#include "bt_grid.hpp"

// == fills.py FILL_KINDS[4..7]
#define DC_FILL_SCHEDULED 4
#define DC_FILL_DIP 5
#define DC_FILL_SCHEDULED_DIP 6
#define DC_FILL_TAKE_PROFIT 7

namespace {

// Where one lane's records and equity samples go. GridLane's recorder as
// it is; DcaFills wraps it.
struct FillWriter {
    float4* __restrict__ rec;      // this lane's max_fills x 2 float4
    float* __restrict__ eq;        // equity + sym * n_samples * P + p
    long eq_step;                  // P
    int max_fills, stride;
    bool act;
    int nrec;                      // fills so far, kept or not
    int cnt;                       // candles since the last equity sample

    __device__ void init(float* records, float* equity, long lane, long pc,
                         int sym, int P, int max_fills_, int stride_,
                         int n_samples, bool act_)
    {
        rec = reinterpret_cast<float4*>(records) + lane * max_fills_ * 2;
        eq = equity + (long)sym * n_samples * P + pc;
        eq_step = P;
        max_fills = max_fills_;
        stride = stride_;
        act = act_;
        nrec = 0;
        cnt = 0;
    }

    __device__ void fill(int t, int kind, int slot, float price, float units,
                         float cash, float pnl, float units_held)
    {
        if (act && nrec < max_fills) {
            rec[2 * (long)nrec] = make_float4(
                __int_as_float(t), __int_as_float(kind),
                __int_as_float(slot), price);
            rec[2 * (long)nrec + 1] =
                make_float4(units, cash, pnl, units_held);
        }
        ++nrec;
    }

    // after the mark to market of each candle
    __device__ void candle(float equity)
    {
        if (++cnt == stride) {
            if (act) *eq = equity;
            eq += eq_step;
            cnt = 0;
        }
    }

    // after the last candle: the final equity sample
    __device__ void finish(float equity)
    {
        if (cnt > 0 && act) *eq = equity;
    }
};

// DcaLane's recorder: names the order and numbers the cycle
struct DcaFills {
    FillWriter w;
    int cycle;                     // take-profits so far

    __device__ void take_profit(int t, float tp_price, float units,
                                float proceeds, float pnl)
    {
        w.fill(t, DC_FILL_TAKE_PROFIT, cycle, tp_price, units, proceeds, pnl,
               0.0f);
        ++cycle;
    }

    __device__ void buy(int t, bool sched, bool dip, float close, float du,
                        float usd, float units)
    {
        const int kind = dip ? (sched ? DC_FILL_SCHEDULED_DIP : DC_FILL_DIP)
                             : DC_FILL_SCHEDULED;
        w.fill(t, kind, cycle, close, du, -usd, 0.0f, units);
    }
};

// LDS as backtest_grid_kernel: 4 blocks/CU is what the table allows
__global__ void __launch_bounds__(BT_BLOCK, 4) backtest_grid_fills_kernel(
    const float* __restrict__ candles,   // (nsym, T, 4)
    const float* __restrict__ pop,       // (P, GR_NPARAM)
    float* __restrict__ metrics,         // (P, nsym, NMETRIC)
    int* __restrict__ n_records,         // (P, nsym)
    float* __restrict__ records,         // (P, nsym, max_fills, 8)
    float* __restrict__ equity,          // (nsym, n_samples, P)
    int nsym, int T, int P, int chunks_per_sym, int max_fills, int stride,
    int n_samples, float initial_equity)
{
#pragma clang fp contract(off)           // match the numpy f32 reference
    __shared__ float lev[GR_NLEV][BT_BLOCK];   // [level][lane]
    __shared__ float4 tile[BT_TILE];           // close, high, low, volume

    int sym, chunk;
    bt_block_map(blockIdx.x, nsym, chunks_per_sym, sym, chunk);
    const int tid = threadIdx.x;
    const int p = chunk * BT_BLOCK + tid;
    const bool act = p < P;
    const long pc = act ? p : 0;         // idle lanes: in-bounds, no stores
    const long lane = pc * nsym + sym;

    GridLane st;
    st.load(pop + pc * GR_NPARAM, initial_equity);
    FillWriter rec;
    rec.init(records, equity, lane, pc, sym, P, max_fills, stride,
             n_samples, act);

    const float4* sym_candles =
        reinterpret_cast<const float4*>(candles + (long)sym * T * 4);

    for (int t0 = 0; t0 < T; t0 += BT_TILE) {
        const int tend = min(BT_TILE, T - t0);
        __syncthreads();
        if (tid < tend) tile[tid] = sym_candles[t0 + tid];
        __syncthreads();
        for (int tt = 0; tt < tend; ++tt) {
            const float4 c = tile[tt];          // b128 broadcast
            const int t = t0 + tt;
            if (t == 0) st.build(lev, tid, t, c.x, rec);
            else st.step(lev, tid, t, c.x, c.y, c.z, rec);
            // --- 4. mark to market -----------------------------------
            st.acc.mark(st.cash + (float)st.units_total * c.x);
            rec.candle(st.acc.equity);
        }
    }

    rec.finish(st.acc.equity);
    if (act) {
        n_records[lane] = rec.nrec;
        st.acc.finalize(metrics + lane * BT_NMETRIC, T);
    }
}

__global__ void __launch_bounds__(BT_BLOCK) backtest_dca_fills_kernel(
    const float* __restrict__ candles,   // (nsym, T, 4)
    const float* __restrict__ pop,       // (P, DC_NPARAM)
    float* __restrict__ metrics,         // (P, nsym, NMETRIC)
    int* __restrict__ n_records,         // (P, nsym)
    float* __restrict__ records,         // (P, nsym, max_fills, 8)
    float* __restrict__ equity,          // (nsym, n_samples, P)
    int nsym, int T, int P, int chunks_per_sym, int max_fills, int stride,
    int n_samples, float initial_equity)
{
#pragma clang fp contract(off)           // match the numpy f32 reference
    __shared__ float chist[DC_SPAN];     // close history incl. halo
    __shared__ float shigh[BT_TILE];
    __shared__ float4 tile[BT_TILE];     // close, high, rmax120, -

    int sym, chunk;
    bt_block_map(blockIdx.x, nsym, chunks_per_sym, sym, chunk);
    const int tid = threadIdx.x;
    const int p = chunk * BT_BLOCK + tid;
    const bool act = p < P;
    const long pc = act ? p : 0;         // idle lanes: in-bounds, no stores
    const long lane = pc * nsym + sym;

    DcaLane st;
    st.load(pop + pc * DC_NPARAM, initial_equity);
    DcaFills rec;
    rec.w.init(records, equity, lane, pc, sym, P, max_fills, stride,
               n_samples, act);
    rec.cycle = 0;

    const float4* sym_candles =
        reinterpret_cast<const float4*>(candles + (long)sym * T * 4);

    for (int t0 = 0; t0 < T; t0 += BT_TILE) {
        const int tend = min(BT_TILE, T - t0);
        dca_stage_tile(sym_candles, t0, T, chist, shigh, tile);
        for (int tt = 0; tt < tend; ++tt) {
            st.step(t0 + tt, tile[tt], rec);     // LDS broadcast reads
            rec.w.candle(st.acc.equity);
        }
    }

    rec.w.finish(st.acc.equity);
    if (act) {
        n_records[lane] = rec.w.nrec;
        st.acc.finalize(metrics + lane * BT_NMETRIC, T);
    }
}

}  // namespace

extern "C" void launch_backtest_grid_fills(
    const float* candles, const float* pop, float* metrics, int* n_records,
    float* records, float* equity, int nsym, int T, int P, int max_fills,
    int stride, int n_samples, float initial_equity, hipStream_t stream)
{
    const int chunks = (P + BT_BLOCK - 1) / BT_BLOCK;
    hipLaunchKernelGGL(backtest_grid_fills_kernel, dim3(nsym * chunks),
                       dim3(BT_BLOCK), 0, stream, candles, pop, metrics,
                       n_records, records, equity, nsym, T, P, chunks,
                       max_fills, stride, n_samples, initial_equity);
}

extern "C" void launch_backtest_dca_fills(
    const float* candles, const float* pop, float* metrics, int* n_records,
    float* records, float* equity, int nsym, int T, int P, int max_fills,
    int stride, int n_samples, float initial_equity, hipStream_t stream)
{
    const int chunks = (P + BT_BLOCK - 1) / BT_BLOCK;
    hipLaunchKernelGGL(backtest_dca_fills_kernel, dim3(nsym * chunks),
                       dim3(BT_BLOCK), 0, stream, candles, pop, metrics,
                       n_records, records, equity, nsym, T, P, chunks,
                       max_fills, stride, n_samples, initial_equity);
}
