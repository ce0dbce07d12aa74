// GPU backtest of the grid-trading family (backtesting/strategy_grid.py is
// the contract; backtesting/engine_grid_cpu.py the numpy twin this kernel
// matches decision-for-decision: fp-contract off, same operation order,
// f64 units_total on both sides).
//
// Skeleton of backtest.hip: 256-lane blocks, one lane per (param-set x
// symbol), every lane of a block on the same symbol, candle tiles staged
// once per block in LDS, XCD-affine block map. No halo: a grid looks at
// the current candle only.
//
// Level table (2H+1 <= 33 f32 per lane) — the decision and its reason:
//   * a register array indexed by a per-lane slot number is dynamically
//     indexed, so the compiler moves all 33 floats to scratch: every
//     level read becomes a scratch (HBM/L2-backed) access on the critical
//     chain. Rejected.
//   * chosen: a [level][lane] table in LDS, 33*256*4 = 33,792 B per block,
//     plus the 4 KB candle tile = 37,888 B. 160 KB of LDS per CU holds 4
//     such blocks = 16 waves/CU = 4 waves/SIMD, which leaves each wave a
//     128-VGPR budget — more than the state needs, so LDS is the one
//     occupancy limiter, at 4 waves/SIMD (the vote kernel runs at 5). A
//     lane only ever touches its own column, address level*256 + lane, so
//     a wave's 64 lanes hit 64 different banks whatever levels they ask
//     for (conflict-free), and the table needs no barrier.
//   * on top of it, a cursor: the two levels that can trigger next — the
//     sell price of the lowest filled slot and the buy price of the
//     highest empty slot — live in registers (sell_px / buy_px), next to
//     the two breakout thresholds. The table is touched only on a candle
//     that crosses one of them.
//
// Mask construction: levels are monotonic, so the sell set is the run of
// filled slots from the bottom whose L[k+1] <= high, and the buy set the
// run of empty slots from the top whose L[k] >= low. The common candle
// crosses nothing: four compares against registers, no table read, no
// slot walk. A crossing candle walks only the slots that actually trade,
// plus one, by ffs/clz over the fill mask.
//
// Compiler resource report (hipcc -O3, gfx950, -Rpass-analysis=
// kernel-resource-usage): 66 VGPR, 0 AGPR, 42 SGPR, 0 B scratch, no
// spills, 37,888 B LDS/block, occupancy 4 waves/SIMD — LDS-limited, as
// the arithmetic above predicts. Measured rates and what bounds them:
// docs/KERNELS.md "Strategy families".
//
// The lane state machine itself (GridLane) is in bt_grid.hpp, shared with
// backtest_fills.hip, which runs it with a recorder that writes one record
// per fill; here it runs with the no-op recorder.

#include "bt_grid.hpp"

namespace {

// min 4 blocks/CU: what the LDS footprint allows (see header)
__global__ void __launch_bounds__(BT_BLOCK, 4) backtest_grid_kernel(
    const float* __restrict__ candles,   // (nsym, T, 4)
    const float* __restrict__ pop,       // (P, GR_NPARAM)
    float* __restrict__ metrics,         // (P, nsym, NMETRIC)
    int nsym, int T, int P, int chunks_per_sym, float initial_equity)
{
#pragma clang fp contract(off)
    __shared__ float lev[GR_NLEV][BT_BLOCK];   // [level][lane]
    __shared__ float4 tile[BT_TILE];           // close, high, low, volume

    int sym, chunk;
    bt_block_map(blockIdx.x, nsym, chunks_per_sym, sym, chunk);
    const int tid = threadIdx.x;
    const int p = chunk * BT_BLOCK + tid;
    const bool act = p < P;

    GridLane st;
    GridNoFills rec;                     // metrics only: no fill records
    st.load(pop + (long)(act ? p : 0) * GR_NPARAM, initial_equity);

    const float4* sym_candles =
        reinterpret_cast<const float4*>(candles + (long)sym * T * 4);

    for (int t0 = 0; t0 < T; t0 += BT_TILE) {
        const int tend = min(BT_TILE, T - t0);
        __syncthreads();
        if (tid < tend) tile[tid] = sym_candles[t0 + tid];
        __syncthreads();
        for (int tt = 0; tt < tend; ++tt) {
            const float4 c = tile[tt];          // b128 broadcast
            if (t0 + tt == 0) st.build(lev, tid, 0, c.x, rec);
            else st.step(lev, tid, t0 + tt, c.x, c.y, c.z, rec);
            // --- 4. mark to market -----------------------------------
            st.acc.mark(st.cash + (float)st.units_total * c.x);
        }
    }

    if (act)
        st.acc.finalize(metrics + ((long)p * nsym + sym) * BT_NMETRIC, T);
}

}  // namespace

extern "C" void launch_backtest_grid(const float* candles, const float* pop,
                                     float* metrics, int nsym, int T, int P,
                                     float initial_equity,
                                     hipStream_t stream) {
    const int chunks = (P + BT_BLOCK - 1) / BT_BLOCK;
    hipLaunchKernelGGL(backtest_grid_kernel, dim3(nsym * chunks),
                       dim3(BT_BLOCK), 0, stream, candles, pop, metrics,
                       nsym, T, P, chunks, initial_equity);
}
