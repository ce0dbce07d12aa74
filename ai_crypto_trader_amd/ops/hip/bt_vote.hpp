// The vote-family contract of backtesting/strategy.py, once, for every
// kernel that implements it (backtest.hip marches it sequentially,
// backtest_tp.hip's bt_flags_kernel time-parallel): constants, parameter
// decode, the per-candle indicator recurrences + six-vote count, the
// Bollinger resnap, and the per-tile LDS staging / shared-series
// precompute. All of it matches backtesting/engine_cpu.py bit for bit
// (fp-contract off, same operation order, f64 Bollinger sums both sides).
#pragma once

#include "bt_common.hpp"

#define BT_NPARAM 19           // == strategy.py NPARAM
#define BT_MAXWIN 32           // == strategy.py MAX_WIN
#define BT_HALO 64             // == strategy.py SHARED_HALO (covers sma50)
#define BT_SPAN (BT_TILE + BT_HALO)
#define BT_WARMUP 128          // == strategy.py WARMUP
#define BT_RESNAP 16384        // == strategy.py RESNAP (BB sum resnap)
// floats per (param, symbol) that bt_trades_kernel carries between its
// chunked launches; ops/backtest.py sizes the carry buffer from it
#define BT_NSTATE 18

// Rolling Bollinger sums of ONE window length w over one close stream,
// and the {mean, std} they give. Nothing here depends on a strategy
// except through w, an integer in [2, BT_MAXWIN]: a kernel may carry one
// per lane (VoteState::step) or one per window for a whole block
// (backtest.hip's table).
struct BollState {
    double sum, sum2, inv_w;          // f64 sums: f32 drifts + cancels

    __device__ void init(int w)
    {
        sum = sum2 = 0.0;
        inv_w = 1.0 / (double)w;
    }

    // Drift-free resnap (strategy.py RESNAP): recompute the window sums
    // directly, oldest->newest, from the close history. `hist` points at
    // close[t] (the resnap candle itself, j = 0 term).
    // (noinline was tried here: 86 VGPR/no spills but the call
    // inside the tile loop cost 25% — inlined + launch-bounds wins)
    __device__ void resnap(int w, const float* __restrict__ hist)
    {
#pragma clang fp contract(off)
        double s = 0.0, s2 = 0.0;
        for (int j = BT_MAXWIN - 1; j >= 0; --j) {
            if (j < w) {
                double c = (double)hist[-j];
                s += c;
                s2 += c * c;
            }
        }
        sum = s;
        sum2 = s2;
    }

    // slide the window one candle: `oldc` is close[t - w], csq_* are
    // (double)close^2 and (double)oldc^2
    __device__ void advance(float close, float oldc, double csq_new,
                            double csq_old)
    {
#pragma clang fp contract(off)
        double old = (double)oldc;
        double c64 = (double)close;
        sum += c64 - old;
        sum2 += csq_new - csq_old;
    }

    // {mean, std} of the window ending at candle t. EARLY = false drops
    // the early-window divisor: a caller that never consumes the entries
    // below t = MAX_WIN gets the same bits everywhere else without
    // carrying the f64 reciprocal.
    template <bool EARLY = true>
    __device__ float2 stats(int t, int w) const
    {
#pragma clang fp contract(off)
        double inv_cnt = inv_w;
        // the early-window divisor only exists in the very first tile
        // (t < MAX_WIN <= 32 < BT_TILE): uniformly skipped t>=32
        if (EARLY && t < BT_MAXWIN && t + 1 < w)
            inv_cnt = 1.0 / (t + 1.0);
        double mean64 = sum * inv_cnt;
        double var64 = fmax(sum2 * inv_cnt - mean64 * mean64, 0.0);
        return make_float2((float)mean64, sqrtf((float)var64));
    }
};

// decoded indicator/vote parameters + recurrence state of one strategy
struct VoteState {
    float inv_rsi_p, rsi_os, rsi_ob;
    float a_f, a_s, a_sig;
    int bb_w;
    float bb_k, bb_bth, bb_sth;
    int entry_v, exit_v;
    float stoch_os, stoch_ob, will_os, will_ob;

    float ema_f, ema_s, sig;
    float avg_gain, avg_loss;
    BollState bb;

    __device__ void load(const float* __restrict__ pr)
    {
        inv_rsi_p = 1.0f / fmaxf(floorf(pr[0]), 1.0f);
        rsi_os = pr[1]; rsi_ob = pr[2];
        a_f = 2.0f / (pr[3] + 1.0f);
        a_s = 2.0f / (pr[4] + 1.0f);
        a_sig = 2.0f / (pr[5] + 1.0f);
        bb_w = min(max((int)pr[6], 2), BT_MAXWIN);
        bb_k = pr[7]; bb_bth = pr[8]; bb_sth = pr[9];
        entry_v = (int)pr[10]; exit_v = (int)pr[11];
        stoch_os = pr[17]; stoch_ob = pr[18];
        will_os = stoch_os - 100.0f;
        will_ob = stoch_ob - 100.0f;
        ema_f = ema_s = sig = 0.f;
        avg_gain = avg_loss = 0.f;
        bb.init(bb_w);
    }

    // Bollinger resnap of this strategy's own window (see BollState)
    __device__ void resnap(const float* __restrict__ hist)
    {
        bb.resnap(bb_w, hist);
    }

    // warm-tail march: the same f32 recurrence ops as step(), minus
    // Bollinger (resnapped at body start) and votes
    __device__ void warm_step(float close, float change)
    {
#pragma clang fp contract(off)
        ema_f += a_f * (close - ema_f);
        ema_s += a_s * (close - ema_s);
        float macd = ema_f - ema_s;
        sig += a_sig * (macd - sig);
        float gain = fmaxf(change, 0.0f);
        float loss = fmaxf(-change, 0.0f);
        avg_gain += (gain - avg_gain) * inv_rsi_p;
        avg_loss += (loss - avg_loss) * inv_rsi_p;
    }

    // step() in three parts, so a kernel may take the Bollinger part
    // from somewhere else (backtest.hip: a block-shared table).
    //
    // Part 1, the O(1) register recurrences of one candle: EMA/MACD and
    // Wilder RSI, as the numerators/denominators the votes compare.
    struct Osc { float macd_hist, rsi_num, rsi_den; };

    // SEEDED: the caller set ema_f = ema_s = close[0] before candle 0, so
    // candle 0 needs no select (backtest_kernel, where the seed is set,
    // says why that gives the same bits), and reads `change` from LDS
    template <bool SEEDED = false>
    __device__ Osc recur(int t, float close, float change)
    {
#pragma clang fp contract(off)           // match the numpy f32 reference
        if (!SEEDED && t == 0) { ema_f = close; ema_s = close; }
        else {
            ema_f += a_f * (close - ema_f);
            ema_s += a_s * (close - ema_s);
        }
        float macd = ema_f - ema_s;
        sig += a_sig * (macd - sig);
        Osc o;
        o.macd_hist = macd - sig;

        // one instruction each for a `change` the caller computed; the
        // seeded caller loads it, which fmaxf would canonicalise first
        float gain = SEEDED ? bt_pos_part(change) : fmaxf(change, 0.0f);
        float loss = SEEDED ? bt_neg_part(change) : fmaxf(-change, 0.0f);
        avg_gain += (gain - avg_gain) * inv_rsi_p;
        avg_loss += (loss - avg_loss) * inv_rsi_p;
        // division-free RSI votes (engine_cpu.py): rsi<thr <=>
        // 100*ag < thr*(ag+al')
        o.rsi_num = 100.0f * avg_gain;
        // (bt_flags_kernel keeps fmaxf: with bt_max its continuous path
        // measured 0.16% slower, profiles/backtest_seg64_lane_loop.json)
        o.rsi_den = avg_gain + (SEEDED ? bt_max_uniform(BT_EPS, avg_loss)
                                       : fmaxf(avg_loss, BT_EPS));
        return o;
    }

    // Part 3, the 6-indicator TradingSignal vote count: net = buys -
    // sells (0 before WARMUP). `ms` is BollState::stats() of this
    // strategy's window at candle t. WARM_TEST = false is for a caller
    // that only comes here with t >= WARMUP. `sv` is the candle's
    // bt_shared_votes entry: {st_num, wl_num, srange, trend}, or with
    // THETA = true the four thresholds of bt_shared_votes<true> and the
    // trend on its own — four compares without their four multiplies.
    template <bool WARM_TEST = true, bool THETA = false>
    __device__ int count(int t, float close, Osc o, float2 ms,
                         float4 sv, int trend = 0) const
    {
#pragma clang fp contract(off)           // match the numpy f32 reference
        float band = bb_k * ms.y;
        // division-free BB votes (engine_cpu.py): pos<thr <=> num<thr*den
        float bb_num = close - (ms.x - band);
        float bb_den = fmaxf(2.0f * band, BT_EPS);

        int net = 0;
        if (!WARM_TEST || t >= BT_WARMUP) {
            int buy = (o.rsi_num < rsi_os * o.rsi_den) +
                      (o.macd_hist > 0.0f) +
                      (bb_num < bb_bth * bb_den);
            int sell = (o.rsi_num > rsi_ob * o.rsi_den) +
                       (o.macd_hist < 0.0f) +
                       (bb_num > bb_sth * bb_den);
            if (THETA) {
                buy += (stoch_os >= sv.x) + (will_os >= sv.z);
                sell += (stoch_ob <= sv.y) + (will_ob <= sv.w);
            } else {
                buy += (sv.x < stoch_os * sv.z) + (sv.y < will_os * sv.z);
                sell += (sv.x > stoch_ob * sv.z) + (sv.y > will_ob * sv.z);
            }
            // sixth vote: the shared trend, already +1 / -1 / 0
            net = buy - sell + (THETA ? trend : __float_as_int(sv.w));
        }
        return net;
    }

    // One candle with a per-lane Bollinger window (part 2 in between):
    // `oldc` is close[t - bb_w]; csq_new / csq_old are (double)close^2
    // and (double)oldc^2, passed in so a caller may share them through
    // LDS. SKIP_BB is a compile-time flag (a resnap() just replaced the
    // sums for this candle) so the steady-state loop carries no
    // per-candle branch — the resnap candle is peeled at the call site.
    template <bool SKIP_BB>
    __device__ int step(int t, float close, float change, float oldc,
                        double csq_new, double csq_old, float4 sv)
    {
        const Osc o = recur(t, close, change);
        // close[t - W] comes from the shared halo tile (== the
        // zero-initialized per-lane ring of engine_cpu.py)
        if (!SKIP_BB) bb.advance(close, oldc, csq_new, csq_old);
        return count(t, close, o, bb.stats(t, bb_w), sv);
    }
};

// Stage candles [t0 - HALO, t0 + TILE) of one symbol into LDS, zero-filled
// outside [0, T): closes into chist, (high, low) into hl and, when csq is
// given, (double)close^2 into csq. Barriers on both sides: the previous
// tile's readers are done before, the tile is visible after. `tid` is
// the thread's index in the block, for a caller that has its own copy.
__device__ inline void bt_stage_tile(
    const float4* __restrict__ sym_candles, int t0, int T,
    float* __restrict__ chist, float (*__restrict__ hl)[2],
    double* __restrict__ csq, int tid = threadIdx.x)
{
#pragma clang fp contract(off)
    __syncthreads();
    for (int i = tid; i < BT_SPAN; i += BT_BLOCK) {
        const int t = t0 - BT_HALO + i;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (t >= 0 && t < T) c = sym_candles[t];
        chist[i] = c.x;
        if (csq) csq[i] = (double)c.x * (double)c.x;
        hl[i][0] = c.y;
        hl[i][1] = c.z;
    }
    __syncthreads();
}

// The ordered-integer image of f32: an involution between a float's bits
// and an int that orders as the floats do, -0 and +0 both at 0. The finite
// floats are [-BT_KEY_INF + 1, BT_KEY_INF - 1]; +-BT_KEY_INF are +-inf.
#define BT_KEY_INF 0x7f800000
__device__ __forceinline__ int bt_key(int k)
{
    return k >= 0 ? k : (int)(0x80000000u - (unsigned)k);
}

// Where a stochastic / Williams vote flips. A lane votes on
// num < fl(p * s) (buy) and num > fl(p * s) (sell) with its own parameter
// p; num and s > 0 belong to the candle. Rounded multiplication by s > 0
// is monotone in p, so Q(p) = SELL ? !(num > fl(p * s)) : num < fl(p * s)
// is false below some float and true from it on. Returns the key of the
// first float with Q true, BT_KEY_INF if no finite one has it. So
//   buy:  num < fl(p * s)  <=>  p >= float(key)
//   sell: num > fl(p * s)  <=>  p <= float(key - 1)    (-inf if none)
// for every finite p. The search probes Q with the very multiply the lanes
// used: it starts at the quotient estimate `est`, gallops off it in
// doubling steps and bisects — two or three probes where the product is a
// normal number, at most 64 wherever it underflows, overflows or the
// estimate is useless. Exact for every finite num and every s > 0.
template <bool SELL>
__device__ inline int bt_vote_flip(float num, float s, float est)
{
#pragma clang fp contract(off)
    auto Q = [&](int k) {
        const float f = __int_as_float(bt_key(k)) * s;
        return SELL ? !(num > f) : (num < f);
    };
    const int KLOW = -BT_KEY_INF, KHIGH = BT_KEY_INF;   // virtual ends
    const int k0 = min(max(bt_key(__float_as_int(est)), KLOW + 1), KHIGH - 1);
    int lo, hi;                       // Q(lo) false, Q(hi) true, or virtual
    unsigned step = 1;
    if (Q(k0)) {
        hi = k0; lo = KLOW;
        while (step < (unsigned)hi - (unsigned)KLOW) {
            const int c = hi - (int)step;
            if (!Q(c)) { lo = c; break; }
            hi = c; step <<= 1;
        }
    } else {
        lo = k0; hi = KHIGH;
        while (step < (unsigned)KHIGH - (unsigned)lo) {
            const int c = lo + (int)step;
            if (Q(c)) { hi = c; break; }
            lo = c; step <<= 1;
        }
    }
    while ((unsigned)hi - (unsigned)lo > 1u) {
        const int mid = lo + (int)(((unsigned)hi - (unsigned)lo) >> 1);
        if (Q(mid)) hi = mid; else lo = mid;
    }
    return hi;
}

// {theta_buy, theta_sell} of one numerator: the lane's buy vote is
// p >= theta_buy, its sell vote p <= theta_sell
__device__ inline float2 bt_vote_thresholds(float num, float s, float inv_s)
{
#pragma clang fp contract(off)
    const float est = num * inv_s;
    return make_float2(
        __int_as_float(bt_key(bt_vote_flip<false>(num, s, est))),
        __int_as_float(bt_key(bt_vote_flip<true>(num, s, est) - 1)));
}

// Param-independent shared vote inputs of tile candles [t0, t0 + tend),
// one thread per candle (strategy.py step-1 spec: every lane of a symbol
// shares them), packed {st_num, wl_num, srange, trend}: st_num =
// 100*(close-lmin14), wl_num = -100*(hmax14-close), srange =
// max(hmax-lmin, eps), trend = the trend vote's buy - sell (+-1/0 from
// close vs sma20/50) as an int's bits, which a lane just adds — so the
// lane loop needs one b128 broadcast read per candle. Finite windows over
// the staged halo: exact wherever the tile starts. The caller's barrier
// publishes sh_vote.
//
// RECORD = true writes one 32-byte record per candle instead, sh_vote
// being [BT_TILE][2]: {close, high, low, change} then the votes, so a lane
// loop reads a whole candle from one address. change = close[t] -
// close[t - 1], 0 at t = 0; the halo holds the previous tile's last close.
// Its votes are not {st_num, wl_num, srange} but where each of the four
// votes on them flips (bt_vote_thresholds): {stoch buy, stoch sell,
// Williams buy, Williams sell}, for VoteState::count<., true> — the
// products p * srange are found once per candle here, not once per lane.
// The record has no room for the trend: it is returned, the calling
// thread's candle's (0 past tend), for the caller to place.
template <bool RECORD = false>
__device__ inline int bt_shared_votes(
    int t0, int tend, const float* __restrict__ chist,
    const float (*__restrict__ hl)[2], float4* __restrict__ sh_vote,
    int tid = threadIdx.x)
{
#pragma clang fp contract(off)
    if (tid >= tend) return 0;
    const int t = t0 + tid;
    const int base = tid + BT_HALO;
    const float cl = chist[base];
    const int L14 = min(t + 1, 14);
    float hmax = -1e30f, lmin = 1e30f;
    for (int j = 0; j < L14; ++j) {
        hmax = fmaxf(hmax, hl[base - j][0]);
        lmin = fminf(lmin, hl[base - j][1]);
    }
    const int L20 = min(t + 1, 20);
    double s20 = 0.0;
    for (int j = 0; j < L20; ++j) s20 += (double)chist[base - j];
    const float sma20 = (float)(s20 / (double)L20);
    const int L50 = min(t + 1, 50);
    double s50 = 0.0;
    for (int j = 0; j < L50; ++j) s50 += (double)chist[base - j];
    const float sma50 = (float)(s50 / (double)L50);
    const int trend = (cl > sma20 && sma20 > sma50) ? 1
                      : ((cl < sma20 && sma20 < sma50) ? -1 : 0);
    const float st_num = 100.0f * (cl - lmin);
    const float wl_num = -100.0f * (hmax - cl);
    const float srange = fmaxf(hmax - lmin, BT_EPS);
    if (RECORD) {
        sh_vote[2 * tid] = make_float4(
            cl, hl[base][0], hl[base][1],
            (t == 0) ? 0.0f : cl - chist[base - 1]);
        const float inv_s = 1.0f / srange;       // an estimate's worth
        const float2 st = bt_vote_thresholds(st_num, srange, inv_s);
        const float2 wl = bt_vote_thresholds(wl_num, srange, inv_s);
        sh_vote[2 * tid + 1] = make_float4(st.x, st.y, wl.x, wl.y);
    } else {
        sh_vote[tid] = make_float4(st_num, wl_num, srange,
                                   __int_as_float(trend));
    }
    return trend;
}
