// Portfolio position machine — the second consumer of bt_flags_kernel's
// bitmaps (backtest_tp.hip): one strategy trades a basket of up to 64
// symbols from ONE cash account with a cap on concurrent positions.
// Contract: backtesting/portfolio.py; numpy twin, bit for bit:
// backtesting/engine_portfolio_cpu.run_portfolio_from_flags_cpu.
//
// One wave per strategy, lane = symbol. What belongs to a symbol (its
// position, its stop / take-profit tests, its four counters) lives in the
// lane; what belongs to the account (cash, open count, the equity / trade
// accumulator, the refusal counts) is wave-uniform: every lane computes
// the same value from kernel arguments and v_readlane broadcasts, so the
// compiler branches on it with scalar branches and the wave never
// diverges on it. That only holds while the candle loop has no divergent
// branch of its own — one makes the structurizer treat the whole loop,
// account included, as divergent — so what a lane does alone is written
// as selects, and the account uses no inline assembly (bt_pf_mark), whose
// results the compiler takes for divergent. Per candle:
//   A. every lane tests its exits at once; the exiting lanes are a ballot,
//      applied to the account bit by bit in ascending lane order with the
//      proceeds / pnl broadcast from the owning lane (exits are rare);
//   B. the candidate ballot likewise, until the slots are used up;
//   C. held = xor-butterfly sum of units * close over the lanes (DPP for
//      the four levels inside a 16-lane row, ds_bpermute for the two
//      across rows) — the balanced tree the contract spells out — then
//      BtAccum::mark.
//
// BT_PF_WAVES strategies share a block and its candle tile: 64 candles of
// every symbol, loaded coalesced along time (a lane's own symbol row sits
// T * 16 bytes from its neighbour's) and laid out [candle][symbol] in LDS
// so the lanes of a wave read one candle from consecutive banks. Each lane
// reads its own two flag words once per tile.
//
// While a strategy is flat and settled (n_open == 0, cash == equity) a
// candle on which no lane has an entry bit changes nothing: equity stays
// cash, r == 0, every accumulator is unchanged (portfolio.py step C with
// held == +0). The wave jumps straight to its next entry bit — the OR of
// the lanes' entry words, found once per tile — or over the whole tile.
//
// The whole candle range runs in one launch.

#include "bt_position.hpp"

#define BT_PF_WAVES 4                      // strategies per block
#define BT_PF_TILE 64                      // candles per tile: a flag word
#define BT_PF_ROW 65                       // padded [candle][symbol] row:
                                           // the staging writes walk banks

namespace {

// x + (x of lane ^ (1 << k)) for k = 0..5: every lane ends with the same
// balanced-tree sum. Inside a 16-lane row the partners come by DPP; after
// level k all 2^(k+1) lanes of a group hold one value, so the mirrors of
// levels 2 and 3 fetch the same operand as lane ^ 4 and lane ^ 8 would.
__device__ __forceinline__ float bt_pf_tree_sum(float x)
{
#pragma clang fp contract(off)
#define BT_PF_DPP(v, ctrl)                                              \
    __int_as_float(__builtin_amdgcn_update_dpp(                         \
        0, __float_as_int(v), (ctrl), 0xf, 0xf, false))
    x += BT_PF_DPP(x, 0xB1);                 // quad_perm [1, 0, 3, 2]
    x += BT_PF_DPP(x, 0x4E);                 // quad_perm [2, 3, 0, 1]
    x += BT_PF_DPP(x, 0x141);                // row_half_mirror
    x += BT_PF_DPP(x, 0x140);                // row_mirror
#undef BT_PF_DPP
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
}

// BtAccum::mark without its inline assembly: the same operations on the
// same values (fmaxf and v_max_f32 agree on everything but signalling NaNs),
// but visibly wave-uniform to the compiler
__device__ __forceinline__ void bt_pf_mark(BtAccum& a, float new_eq)
{
#pragma clang fp contract(off)
    const float r = new_eq / a.equity - 1.0f;
    a.sum_ret += r;
    a.sum_ret2 += r * r;
    a.equity = new_eq;
    a.max_eq = fmaxf(a.max_eq, new_eq);
    const float x = a.max_eq - new_eq;       // BtAccum::mark's guard
    if (!(x <= a.max_eq * (a.dd_c * a.max_dd)))
        a.max_dd = fmaxf(a.max_dd, x / a.max_eq);
}

__device__ __forceinline__ float bt_pf_readlane(float v, int lane)
{
    return __int_as_float(
        __builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__device__ __forceinline__ unsigned long long bt_pf_uniform(
    unsigned long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// OR of a word over the wave, wave-uniform
__device__ __forceinline__ unsigned long long bt_pf_wave_or(
    unsigned long long v)
{
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    for (int m = 1; m < 64; m <<= 1) {
        lo |= (unsigned)__shfl_xor((int)lo, m);
        hi |= (unsigned)__shfl_xor((int)hi, m);
    }
    return bt_pf_uniform(((unsigned long long)hi << 32) | lo);
}

__global__ void __launch_bounds__(BT_PF_WAVES * 64) bt_portfolio_kernel(
    const float* __restrict__ candles,             // (nsym, T, 4)
    const float* __restrict__ pop,                 // (P, NPARAM)
    const unsigned long long* __restrict__ eflags,  // (nsym, nwords, P)
    const unsigned long long* __restrict__ xflags,
    float* __restrict__ metrics,                   // (P, NMETRIC)
    float* __restrict__ per_symbol,                // (P, nsym, 4)
    int* __restrict__ refused,                     // (P, 2)
    float* __restrict__ equity_out,                // (P, n_samples) or null
    int nsym, int T, int P, int max_positions, float initial_equity,
    int stride, int n_samples)
{
#pragma clang fp contract(off)
    __shared__ float sc[BT_PF_TILE][BT_PF_ROW];
    __shared__ float sh[BT_PF_TILE][BT_PF_ROW];
    __shared__ float sl[BT_PF_TILE][BT_PF_ROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int p = __builtin_amdgcn_readfirstlane(
        blockIdx.x * BT_PF_WAVES + (tid >> 6));
    const bool wact = p < P;                 // the wave has a strategy
    const bool act = wact && lane < nsym;    // the lane has a symbol
    const long nwords = (T + 63) >> 6;
    const bool record = stride > 0;

    // strategy parameters: wave-uniform
    const float* pr = pop + (long)(wact ? p : 0) * BT_NPARAM;
    const float size_pct = pr[12];
    const float fee_m = 1.0f - BT_FEE;
    const float sl_m = 1.0f - pr[13];
    const float tp_m = 1.0f + pr[14];
    const float trail_m = 1.0f - pr[15];
    const float act_m = 1.0f + pr[16];
    const bool trail_en = pr[15] > 0.0f;

    // the account: wave-uniform
    float cash = initial_equity;
    int n_open = 0, ref_slots = 0, ref_cash = 0;
    BtAccum acc;
    acc.init(initial_equity);

    // the lane's symbol
    float units = 0.f, entry_cost = 0.f, trail_trig = 0.f;
    float stop = 0.f, tp = 0.f, peak = 0.f;
    bool in_pos = false;
    float s_trades = 0.f, s_wins = 0.f, s_gp = 0.f, s_gl = 0.f;

    const unsigned long long* my_e =
        eflags + (long)(act ? lane : 0) * nwords * P + (wact ? p : 0);
    const unsigned long long* my_x =
        xflags + (long)(act ? lane : 0) * nwords * P + (wact ? p : 0);
    const float4* c4 = reinterpret_cast<const float4*>(candles);
    float* my_eq = record ? equity_out + (long)(wact ? p : 0) * n_samples
                          : nullptr;

    for (int t0 = 0; t0 < T; t0 += BT_PF_TILE) {
        const int hlen = min(BT_PF_TILE, T - t0);

        // stage the tile: consecutive threads walk one symbol's candles
        __syncthreads();                     // the last tile's readers
        for (int i = tid; i < nsym * BT_PF_TILE; i += BT_PF_WAVES * 64) {
            const int s = i >> 6, k = i & 63;
            if (k < hlen) {
                const float4 c = c4[(long)s * T + t0 + k];
                sc[k][s] = c.x;
                sh[k][s] = c.y;
                sl[k][s] = c.z;
            }
        }
        __syncthreads();
        if (!wact) continue;

        const long w = t0 >> 6;
        unsigned long long ew = act ? my_e[w * P] : 0ull;
        unsigned long long xw = act ? my_x[w * P] : 0ull;
        if (hlen < 64) ew &= (1ull << hlen) - 1ull;   // bits past T: none
        const unsigned long long eany = bt_pf_wave_or(ew);

        float eq_hold = acc.equity;          // lane k: equity after t0 + k

        int k = 0;
        while (k < hlen) {
            if (n_open == 0 && cash == acc.equity) {
                // flat and settled: nothing happens before the next
                // entry bit of any lane
                const unsigned long long rest = eany >> k;
                const int skip =
                    rest ? min(__builtin_ctzll(rest), hlen - k) : hlen - k;
                if (skip > 0) {
                    eq_hold = (record && lane >= k && lane < k + skip)
                                  ? acc.equity : eq_hold;
                    k += skip;
                    continue;
                }
            }

            const float close = sc[k][lane];
            const float high = sh[k][lane];
            const float low = sl[k][lane];
            const bool ebit = (ew >> k) & 1ull;
            const bool xbit = (xw >> k) & 1ull;
            const bool pos0 = in_pos;

            // --- A. exits ------------------------------------------------
            if (n_open > 0) {
                peak = pos0 ? bt_max(peak, high) : peak;
                const bool trail_on =
                    pos0 && trail_en && peak >= trail_trig;
                stop = trail_on ? bt_max(stop, peak * trail_m) : stop;
                const bool hit_sl = pos0 && low <= stop;
                const bool hit_tp = pos0 && !hit_sl && high >= tp;
                const bool exiting = hit_sl || hit_tp || (pos0 && xbit);
                unsigned long long xmask = __ballot(exiting);
                if (xmask) {
                    const float price = hit_sl ? stop : (hit_tp ? tp : close);
                    const float proceeds = units * price * fee_m;
                    const float pnl = proceeds - entry_cost;
                    s_trades += exiting ? 1.0f : 0.0f;
                    s_wins += (exiting && pnl > 0.0f) ? 1.0f : 0.0f;
                    s_gp += exiting ? fmaxf(pnl, 0.0f) : 0.0f;
                    s_gl += exiting ? fmaxf(-pnl, 0.0f) : 0.0f;
                    units = exiting ? 0.0f : units;
                    in_pos = pos0 && !exiting;
                    do {                     // ascending symbol index
                        const int s = __builtin_ctzll(xmask);
                        xmask &= xmask - 1ull;
                        cash += bt_pf_readlane(proceeds, s);
                        acc.trade(bt_pf_readlane(pnl, s));
                        n_open -= 1;
                    } while (xmask);
                }
            }

            // --- B. entries ----------------------------------------------
            unsigned long long cmask = __ballot(!pos0 && ebit);
            while (cmask) {
                if (n_open >= max_positions) {
                    ref_slots += __builtin_popcountll(cmask);
                    break;
                }
                const int s = __builtin_ctzll(cmask);
                cmask &= cmask - 1ull;
                const float cost = fminf(size_pct * acc.equity, cash);
                if (cost <= 0.0f) {
                    ref_cash += 1;
                    continue;
                }
                cash -= cost;
                n_open += 1;
                const bool mine = lane == s;
                units = mine ? cost * fee_m / close : units;
                entry_cost = mine ? cost : entry_cost;
                trail_trig = mine ? close * act_m : trail_trig;
                stop = mine ? close * sl_m : stop;
                tp = mine ? close * tp_m : tp;
                peak = mine ? close : peak;
                in_pos = in_pos || mine;
            }

            // --- C. mark -------------------------------------------------
            const float held =
                bt_pf_tree_sum(in_pos ? units * close : 0.0f);
            bt_pf_mark(acc, cash + bt_pf_readlane(held, 0));
            eq_hold = (record && lane == k) ? acc.equity : eq_hold;
            ++k;
        }

        if (record) {
            // ledger.py's sampling: sample j is the equity after candle
            // min((j + 1) * stride - 1, T - 1)
            const int t = t0 + lane;
            if (lane < hlen && ((t + 1) % stride == 0 || t == T - 1))
                my_eq[t / stride] = eq_hold;
        }
    }

    if (!wact) return;
    if (act)
        reinterpret_cast<float4*>(per_symbol)[(long)p * nsym + lane] =
            make_float4(s_trades, s_wins, s_gp, s_gl);
    if (lane == 0) {
        acc.finalize(metrics + (long)p * BT_NMETRIC, T);
        refused[2 * (long)p] = ref_slots;
        refused[2 * (long)p + 1] = ref_cash;
    }
}

}  // namespace

extern "C" void launch_bt_portfolio(
    const float* candles, const float* pop,
    const unsigned long long* eflags, const unsigned long long* xflags,
    float* metrics, float* per_symbol, int* refused, float* equity,
    int nsym, int T, int P, int max_positions, float initial_equity,
    int stride, int n_samples, hipStream_t stream)
{
    const int blocks = (P + BT_PF_WAVES - 1) / BT_PF_WAVES;
    hipLaunchKernelGGL(bt_portfolio_kernel, dim3(blocks),
                       dim3(BT_PF_WAVES * 64), 0, stream, candles, pop,
                       eflags, xflags, metrics, per_symbol, refused, equity,
                       nsym, T, P, max_positions, initial_equity, stride,
                       n_samples);
}
