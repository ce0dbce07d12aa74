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

#include "bt_common.hpp"

#define GR_NPARAM 5
#define GR_MAXHALF 16            // == strategy_grid.py MAX_HALF
#define GR_NLEV (2 * GR_MAXHALF + 1)

namespace {

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

    __device__ void build(float (*lev)[BT_BLOCK], int tid, float close)
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
        filled = slotmask & ~((1u << H) - 1u);
        initial = filled;
        up_thr = up * up_k;
        dn_thr = dn * dn_k;
        refresh_px(lev, tid);
    }

    __device__ void step(float (*lev)[BT_BLOCK], int tid, float close,
                         float high, float low)
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
                units_total += (double)(bomf / lk);
                filled |= 1u << k;
                initial &= ~(1u << k);
                m &= ~(1u << k);
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
            }
            build(lev, tid, close);
        } else if (touched) {
            refresh_px(lev, tid);
        }
    }
};

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
            if (t0 + tt == 0) st.build(lev, tid, c.x);
            else st.step(lev, tid, c.x, c.y, c.z);
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
