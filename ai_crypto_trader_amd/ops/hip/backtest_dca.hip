// GPU backtest of the dollar-cost-averaging family
// (backtesting/strategy_dca.py is the contract;
// backtesting/engine_dca_cpu.py the numpy twin this kernel matches
// decision-for-decision: fp-contract off, same operation order).
//
// Skeleton of backtest.hip: 256-lane blocks, one lane per (param-set x
// symbol), every lane of a block on the same symbol, candle tiles staged
// once per block in LDS, XCD-affine block map.
//
// rmax120 (the dip reference, max close over the last 120 candles) — the
// decision and its reason: it is parameter-independent, so it is computed
// cooperatively per tile from a 128-candle close halo in LDS, one thread
// per tile candle, exactly as backtest.hip derives hmax14/sma50 from its
// 64-candle halo. Cost: 120 LDS reads per thread per 256-candle tile,
// under half a read per candle-eval, for 1.5 KB of halo. The alternative,
// a per-symbol pre-pass into an (nsym, T) buffer, would add a second
// launch, a 4 B/candle HBM round trip and an allocation to every call
// for nothing: max is exact and order-free, so both give identical bits.
// The lane loop then gets {close, high, rmax120} in one b128 broadcast.
//
// The schedule test n % period == 0 is a per-lane counter pair (`since`
// counts n mod period, `nper` counts n / period), not an integer modulo
// per candle — gfx950 has no integer divide.
//
// Compiler resource report (hipcc -O3, gfx950, -Rpass-analysis=
// kernel-resource-usage): 50 VGPR, 0 AGPR, 42 SGPR, 0 B scratch, no
// spills, 6,656 B LDS/block, occupancy 8 waves/SIMD. Measured rates:
// docs/KERNELS.md "Strategy families".
//
// The lane state machine itself (DcaLane) is in bt_dca.hpp, shared with
// backtest_fills.hip, which runs it with a recorder that writes one record
// per order; here it runs with the no-op recorder.

#include "bt_dca.hpp"

namespace {

__global__ void __launch_bounds__(BT_BLOCK) backtest_dca_kernel(
    const float* __restrict__ candles,   // (nsym, T, 4)
    const float* __restrict__ pop,       // (P, DC_NPARAM)
    float* __restrict__ metrics,         // (P, nsym, NMETRIC)
    int nsym, int T, int P, int chunks_per_sym, float initial_equity)
{
#pragma clang fp contract(off)           // match the numpy f32 reference
    __shared__ float chist[DC_SPAN];     // close history incl. halo
    __shared__ float shigh[BT_TILE];
    __shared__ float4 tile[BT_TILE];    // close, high, rmax120, -

    int sym, chunk;
    bt_block_map(blockIdx.x, nsym, chunks_per_sym, sym, chunk);
    const int tid = threadIdx.x;
    const int p = chunk * BT_BLOCK + tid;
    const bool act = p < P;

    DcaLane st;
    DcaNoFills rec;                      // metrics only: no fill records
    st.load(pop + (long)(act ? p : 0) * DC_NPARAM, initial_equity);

    const float4* sym_candles =
        reinterpret_cast<const float4*>(candles + (long)sym * T * 4);

    for (int t0 = 0; t0 < T; t0 += BT_TILE) {
        const int tend = min(BT_TILE, T - t0);
        // bt_dca.hpp's dca_stage_tile, kept in the body (the reason is
        // there)
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
        for (int tt = 0; tt < tend; ++tt)
            st.step(t0 + tt, tile[tt], rec);     // LDS broadcast reads
    }

    if (act)
        st.acc.finalize(metrics + ((long)p * nsym + sym) * BT_NMETRIC, T);
}

}  // namespace

extern "C" void launch_backtest_dca(const float* candles, const float* pop,
                                    float* metrics, int nsym, int T, int P,
                                    float initial_equity,
                                    hipStream_t stream) {
    const int chunks = (P + BT_BLOCK - 1) / BT_BLOCK;
    hipLaunchKernelGGL(backtest_dca_kernel, dim3(nsym * chunks),
                       dim3(BT_BLOCK), 0, stream, candles, pop, metrics,
                       nsym, T, P, chunks, initial_equity);
}
