// Market-regime stack (PARITY.md §2.9, services/market_regime.py): window
// features, the Gaussian-HMM E-step and Viterbi for B sequences at once.
// CPU twins and the wrappers: ops/regime.py.
//
// regime_features_kernel
//   One block owns 256 consecutive windows of one symbol and stages the
//   256 + win closes they cover, and their log-returns, in LDS once. A
//   thread owns one window and walks it twice: lane l reads sc[l + k], so
//   every LDS read is stride-1 over the wave (conflict-free). Prices sit
//   at levels like 6e4 where f32 has ~3 decimals left for a window's
//   spread, so every sum is taken about a pivot: pass 1 sums w[k] - w[-1],
//   pass 2 sums the deviations from the window mean.
//
// hmm_estep_kernel / hmm_viterbi_kernel
//   One wavefront per sequence, lane = i * 8 + j for the K x K (K <= 8)
//   transition products; lanes with i >= K or j >= K carry zeros. The
//   recursion is sequential in t. Reductions over i are __shfl_xor with
//   8/16/32, over j with 1/2/4; the transpose between "indexed by j" and
//   "indexed by i" is one __shfl. All control flow is wave-uniform.
//
//   Forward: scaled (Rabiner) recursion. Each step's emission
//   log-densities are shifted by their max over states before exp2, and
//   log c_t + shift_t goes into the log-likelihood: K exp and one log per
//   step. Emissions are recomputed from mu/var in both passes; no (T, K)
//   emission tensor goes through memory. Backward: beta lives in
//   registers; xi_sum[i][j] accumulates in lane (i, j) and sx/sxx[i][f]
//   in lane (i, f). gamma_t and xi_t are divided by sum_i alpha_t[i]
//   beta_t[i], which removes the common-mode drift of the carried beta.

#include "common.hpp"

#include <cfloat>

namespace {

constexpr int FEAT_TILE = 256;
constexpr int FEAT_MAXWIN = 256;
constexpr int HMM_MAXK = 8;
constexpr int HMM_MAXF = 8;
constexpr int HMM_WAVES = 4;           // sequences per block
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// ---------------------------------------------------------------------------
// features
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(FEAT_TILE) regime_features_kernel(
    const float* __restrict__ closes,   // (S, Tmax)
    const int* __restrict__ lengths,    // (S,)
    float* __restrict__ out,            // (S, Tmax - win, 6)
    int Tmax, int win)
{
    __shared__ float sc[FEAT_TILE + FEAT_MAXWIN];
    __shared__ float sr[FEAT_TILE + FEAT_MAXWIN];
    const int s = blockIdx.y;
    const int tile0 = blockIdx.x * FEAT_TILE;
    const int nw = Tmax - win;
    const int len = min(max(lengths[s], 0), Tmax);
    const int nvalid = len - win;       // windows this symbol really has
    const int i = tile0 + (int)threadIdx.x;
    float* o = out + ((size_t)s * nw + i) * 6;

    if (nvalid <= tile0) {              // block-uniform: nothing to stage
        if (i < nw) {
#pragma unroll
            for (int f = 0; f < 6; ++f) o[f] = 0.0f;
        }
        return;
    }
    const float* c = closes + (size_t)s * Tmax;
    const int nstage = FEAT_TILE + win;
    for (int j = threadIdx.x; j < nstage; j += FEAT_TILE)
        sc[j] = c[min(tile0 + j, len - 1)];
    __syncthreads();
    for (int j = threadIdx.x; j < nstage - 1; j += FEAT_TILE) {
        const float a = sc[j];
        sr[j] = log1pf((sc[j + 1] - a) / a);
    }
    __syncthreads();
    if (i >= nw) return;
    if (i >= nvalid) {
#pragma unroll
        for (int f = 0; f < 6; ++f) o[f] = 0.0f;
        return;
    }

    const float* w = sc + threadIdx.x;
    const float* r = sr + threadIdx.x;
    const float p = w[win - 1];
    const int kf = win - min(win, 12);
    const int ks = win >= 26 ? win - 26 : 0;
    float S = 0.f, Sf = 0.f, Ss = 0.f, G = 0.f, L = 0.f, R = 0.f;
    float prev = w[0];
    for (int k = 0; k < win; ++k) {
        const float wk = w[k];
        const float d = wk - p;
        S += d;
        if (k >= kf) Sf += d;
        if (k >= ks) Ss += d;
        const float df = wk - prev;     // 0 at k == 0
        G += fmaxf(df, 0.0f);
        L += fmaxf(-df, 0.0f);
        if (k < win - 1) R += r[k];
        prev = wk;
    }
    const float fwin = (float)win;
    const float nr = (float)(win - 1);
    const float dm = S / fwin;          // mean - p
    const float rm = R / nr;
    const float xbar = 0.5f * (fwin - 1.0f);
    float E2 = 0.f, XE = 0.f, R2 = 0.f;
    for (int k = 0; k < win; ++k) {
        const float e = (w[k] - p) - dm;
        E2 = fmaf(e, e, E2);
        XE = fmaf((float)k - xbar, e, XE);
        if (k < win - 1) {
            const float q = r[k] - rm;
            R2 = fmaf(q, q, R2);
        }
    }
    const float mean = p + dm;
    const float sxx = fwin * (fwin * fwin - 1.0f) * (1.0f / 12.0f);
    const float g = G / nr, l = L / nr;
    o[0] = p / w[0] - 1.0f;
    o[1] = sqrtf(R2 / nr);
    o[2] = XE / sxx / mean * fwin;
    o[3] = 100.0f * g / fmaxf(g + l, 1e-12f);
    o[4] = (Sf / (float)(win - kf) - Ss / (float)(win - ks)) / p;
    o[5] = sqrtf(E2 / fwin) / fmaxf(mean, 1e-9f);
}

// ---------------------------------------------------------------------------
// HMM helpers
// ---------------------------------------------------------------------------
DEV_INLINE float bcast(float v, int lane) {     // lane: compile-time constant
    return __int_as_float(
        __builtin_amdgcn_readlane(__float_as_int(v), lane));
}

DEV_INLINE float sum_over_j(float v) {
    v += __shfl_xor(v, 1, WAVE);
    v += __shfl_xor(v, 2, WAVE);
    v += __shfl_xor(v, 4, WAVE);
    return v;
}

DEV_INLINE float max_over_j(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, WAVE));
    v = fmaxf(v, __shfl_xor(v, 2, WAVE));
    v = fmaxf(v, __shfl_xor(v, 4, WAVE));
    return v;
}

DEV_INLINE float sum_over_i(float v) {
    v += __shfl_xor(v, 8, WAVE);
    v += __shfl_xor(v, 16, WAVE);
    v += __shfl_xor(v, 32, WAVE);
    return v;
}

// State j's diagonal Gaussian, held by every lane of column j.
struct Emission {
    float mu[HMM_MAXF];
    float iv[HMM_MAXF];     // 1 / var
    float hd;               // -0.5 * sum_f log var; -inf in lanes j >= K

    DEV_INLINE void load(const float* __restrict__ mu_b,
                         const float* __restrict__ var_b, int j, int K,
                         int F) {
        float ld = 0.0f;
#pragma unroll
        for (int f = 0; f < HMM_MAXF; ++f) {
            mu[f] = 0.0f;
            iv[f] = 0.0f;
            if (f < F && j < K) {
                const float v = var_b[j * F + f];
                mu[f] = mu_b[j * F + f];
                iv[f] = 1.0f / v;
                ld += __builtin_amdgcn_logf(v) * LN2;
            }
        }
        hd = j < K ? -0.5f * ld : -INFINITY;
    }

    // xv: lane l < F holds x_t[l]
    DEV_INLINE float logb(float xv, int F) const {
        float q = 0.0f;
#pragma unroll
        for (int f = 0; f < HMM_MAXF; ++f) {
            if (f < F) {
                const float d = bcast(xv, f) - mu[f];
                q = fmaf(d * d, iv[f], q);
            }
        }
        return fmaf(-0.5f, q, hd);
    }
};

DEV_INLINE float exp_shifted(float logb, float mx) {
    return __builtin_amdgcn_exp2f((logb - mx) * LOG2E);
}

// ---------------------------------------------------------------------------
// E-step
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(HMM_WAVES * WAVE) hmm_estep_kernel(
    const float* __restrict__ X,        // (B, Tmax, F)
    const int* __restrict__ lengths,    // (B,)
    const float* __restrict__ mu,       // (B, K, F)
    const float* __restrict__ var,      // (B, K, F)
    const float* __restrict__ logA,     // (B, K, K)
    const float* __restrict__ logpi,    // (B, K)
    float* alpha_ws,                    // (B, Tmax, K) scaled alpha
    float* c_ws,                        // (B, Tmax)    scale c_t
    float* __restrict__ ll,             // (B,)
    float* __restrict__ gamma0,         // (B, K)
    float* __restrict__ gamma_sum,      // (B, K)
    float* __restrict__ gamma_head,     // (B, K) sum over t < T-1
    float* __restrict__ xi_sum,         // (B, K, K)
    float* __restrict__ sx,             // (B, K, F)
    float* __restrict__ sxx,            // (B, K, F)
    float* __restrict__ gamma,          // (B, Tmax, K) or nullptr
    int B, int Tmax, int K, int F)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * HMM_WAVES + (int)(threadIdx.x / WAVE);
    if (b >= B) return;                 // wave-uniform
    const int i = lane >> 3, j = lane & 7;
    const bool act = i < K && j < K;
    const bool col = i == 0 && j < K;   // the lanes that own "indexed by j"
    const bool row = j == 0 && i < K;   // ... and "indexed by i"
    const int len = min(max(lengths[b], 0), Tmax);

    const float* Xb = X + (size_t)b * Tmax * F;
    float* ab = alpha_ws + (size_t)b * Tmax * K;
    float* cb = c_ws + (size_t)b * Tmax;
    float* gb = gamma ? gamma + (size_t)b * Tmax * K : nullptr;

    if (gb) {
        for (int q = len * K + lane; q < Tmax * K; q += WAVE) gb[q] = 0.0f;
    }
    if (len == 0) {
        if (lane == 0) ll[b] = 0.0f;
        if (col) {
            gamma0[b * K + j] = 0.0f;
            gamma_sum[b * K + j] = 0.0f;
            gamma_head[b * K + j] = 0.0f;
        }
        if (act) xi_sum[(b * K + i) * K + j] = 0.0f;
        if (i < K && j < F) {
            sx[(b * K + i) * F + j] = 0.0f;
            sxx[(b * K + i) * F + j] = 0.0f;
        }
        return;
    }

    Emission em;
    em.load(mu + (size_t)b * K * F, var + (size_t)b * K * F, j, K, F);
    const float A = act
        ? __builtin_amdgcn_exp2f(logA[(b * K + i) * K + j] * LOG2E) : 0.0f;

    // ---- forward ----------------------------------------------------------
    double llacc = 0.0;
    float ai = 0.0f;                    // alpha_{t-1}[i]
    {
        const float pj = j < K
            ? __builtin_amdgcn_exp2f(logpi[b * K + j] * LOG2E) : 0.0f;
        float xv = j < F ? Xb[j] : 0.0f;
        float xn = (j < F && len > 1) ? Xb[F + j] : 0.0f;
        for (int t = 0; t < len; ++t) {
            const float lb = em.logb(xv, F);
            const float mx = max_over_j(lb);
            const float bj = exp_shifted(lb, mx);
            const float pred = t == 0 ? pj : sum_over_i(ai * A);
            const float au = pred * bj;
            const float c = fmaxf(sum_over_j(au), FLT_MIN);
            const float aj = au * __builtin_amdgcn_rcpf(c);
            llacc += (double)(__builtin_amdgcn_logf(c) * LN2 + mx);
            if (col) ab[t * K + j] = aj;
            if (lane == 0) cb[t] = c;
            ai = __shfl(aj, i, WAVE);
            xv = xn;
            if (j < F && t + 2 < len) xn = Xb[(size_t)(t + 2) * F + j];
        }
    }
    if (lane == 0) ll[b] = (float)llacc;
    // alpha and c were written by other lanes of this wave
    __threadfence();

    // ---- backward ---------------------------------------------------------
    float xi = 0.0f, gs = 0.0f, gh = 0.0f, ax = 0.0f, axx = 0.0f;
    float g0 = 0.0f;
    {
        int t = len - 1;
        float xv = j < F ? Xb[(size_t)t * F + j] : 0.0f;
        float a_t = i < K ? ab[t * K + i] : 0.0f;
        float gam = a_t / fmaxf(sum_over_i(a_t), FLT_MIN);
        gs += gam;
        ax = fmaf(gam, xv, ax);
        axx = fmaf(gam * xv, xv, axx);
        if (gb && row) gb[t * K + i] = gam;
        if (t == 0) g0 = gam;
        float bc = j < K ? 1.0f : 0.0f;         // beta_t[j]

        // operands of the step t -> t-1, loaded one step ahead
        int tp = max(t - 1, 0);
        float xp = j < F ? Xb[(size_t)tp * F + j] : 0.0f;
        float ap = i < K ? ab[tp * K + i] : 0.0f;
        float ct = cb[t];
        for (; t >= 1; --t) {
            const int tq = max(t - 2, 0);
            const float xq = j < F ? Xb[(size_t)tq * F + j] : 0.0f;
            const float aq = i < K ? ab[tq * K + i] : 0.0f;
            const float cq = cb[t - 1];

            const float lb = em.logb(xv, F);
            const float mx = max_over_j(lb);
            const float bj = exp_shifted(lb, mx);
            const float w = A * (bj * bc) * __builtin_amdgcn_rcpf(ct);
            const float br = sum_over_j(w);     // beta_{t-1}[i]
            const float gu = ap * br;
            const float rg = 1.0f / fmaxf(sum_over_i(gu), FLT_MIN);
            gam = gu * rg;
            xi = fmaf(ap * w, rg, xi);
            gs += gam;
            gh += gam;
            ax = fmaf(gam, xp, ax);
            axx = fmaf(gam * xp, xp, axx);
            if (gb && row) gb[(t - 1) * K + i] = gam;
            if (t == 1) g0 = gam;
            bc = __shfl(br, j * 8, WAVE);
            xv = xp;
            xp = xq;
            ap = aq;
            ct = cq;
        }
    }
    if (row) {
        gamma0[b * K + i] = g0;
        gamma_sum[b * K + i] = gs;
        gamma_head[b * K + i] = gh;
    }
    if (act) xi_sum[(b * K + i) * K + j] = xi;
    if (i < K && j < F) {
        sx[(b * K + i) * F + j] = ax;
        sxx[(b * K + i) * F + j] = axx;
    }
}

// ---------------------------------------------------------------------------
// Viterbi
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(HMM_WAVES * WAVE) hmm_viterbi_kernel(
    const float* __restrict__ X, const int* __restrict__ lengths,
    const float* __restrict__ mu, const float* __restrict__ var,
    const float* __restrict__ logA, const float* __restrict__ logpi,
    unsigned char* bp_ws,               // (B, Tmax, K) back-pointers
    int* __restrict__ path,             // (B, Tmax), -1 past lengths[b]
    int B, int Tmax, int K, int F)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * HMM_WAVES + (int)(threadIdx.x / WAVE);
    if (b >= B) return;
    const int i = lane >> 3, j = lane & 7;
    const bool act = i < K && j < K;
    const bool col = i == 0 && j < K;
    const int len = min(max(lengths[b], 0), Tmax);
    const float* Xb = X + (size_t)b * Tmax * F;
    unsigned char* bpb = bp_ws + (size_t)b * Tmax * K;
    int* pb = path + (size_t)b * Tmax;

    for (int t = len + lane; t < Tmax; t += WAVE) pb[t] = -1;
    if (len == 0) return;

    Emission em;
    em.load(mu + (size_t)b * K * F, var + (size_t)b * K * F, j, K, F);
    const float lA = act ? logA[(b * K + i) * K + j] : -INFINITY;

    float dj = 0.0f;                    // delta_t[j]
    float di = 0.0f;                    // delta_{t-1}[i]
    float xv = j < F ? Xb[j] : 0.0f;
    float xn = (j < F && len > 1) ? Xb[F + j] : 0.0f;
    for (int t = 0; t < len; ++t) {
        const float lb = em.logb(xv, F);
        if (t == 0) {
            dj = (j < K ? logpi[b * K + j] : -INFINITY) + lb;
        } else {
            float v = di + lA;
            int idx = i;
#pragma unroll
            for (int off = 8; off < WAVE; off <<= 1) {
                const float ov = __shfl_xor(v, off, WAVE);
                const int oi = __shfl_xor(idx, off, WAVE);
                // ties go to the lowest state, as np.argmax does
                if (ov > v || (ov == v && oi < idx)) {
                    v = ov;
                    idx = oi;
                }
            }
            dj = v + lb;
            if (col) bpb[(size_t)t * K + j] = (unsigned char)idx;
        }
        // paths are invariant to a per-step shift; it keeps delta near 0
        // where f32 resolves the differences between states
        dj -= max_over_j(dj);
        di = __shfl(dj, i, WAVE);
        xv = xn;
        if (j < F && t + 2 < len) xn = Xb[(size_t)(t + 2) * F + j];
    }

    // argmax_j delta_{T-1}[j], lowest index on ties
    int state = j;
    {
        float v = j < K ? dj : -INFINITY;
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            const float ov = __shfl_xor(v, off, WAVE);
            const int oi = __shfl_xor(state, off, WAVE);
            if (ov > v || (ov == v && oi < state)) {
                v = ov;
                state = oi;
            }
        }
        state = __builtin_amdgcn_readfirstlane(state);
    }
    // the back-pointers were written by other lanes of this wave
    __threadfence();

    // backtrack, 64 steps per round: lane l packs step (base - l)'s K
    // back-pointers into 3 bits each, the walk itself is scalar
    for (int base = len - 1; base >= 0; base -= WAVE) {
        const int t = base - lane;
        unsigned wd = 0;
        if (t >= 1) {
#pragma unroll
            for (int k = 0; k < HMM_MAXK; ++k)
                if (k < K) wd |= (unsigned)bpb[(size_t)t * K + k] << (3 * k);
        }
        const int n = min(WAVE, base + 1);
        int mine = 0;
        for (int l = 0; l < n; ++l) {
            if (lane == l) mine = state;
            const unsigned wl =
                (unsigned)__builtin_amdgcn_readlane((int)wd, l);
            state = (int)((wl >> (3 * state)) & 7u);
        }
        if (t >= 0) pb[t] = mine;
    }
}

}  // namespace

extern "C" void launch_regime_features(const float* closes,
                                       const int* lengths, float* out,
                                       int S, int Tmax, int win,
                                       hipStream_t stream) {
    const int nw = Tmax - win;
    if (nw <= 0 || S <= 0) return;
    dim3 grid((nw + FEAT_TILE - 1) / FEAT_TILE, S);
    hipLaunchKernelGGL(regime_features_kernel, grid, dim3(FEAT_TILE), 0,
                       stream, closes, lengths, out, Tmax, win);
}

extern "C" void launch_hmm_estep(
    const float* X, const int* lengths, const float* mu, const float* var,
    const float* logA, const float* logpi, float* alpha_ws, float* c_ws,
    float* ll, float* gamma0, float* gamma_sum, float* gamma_head,
    float* xi_sum, float* sx, float* sxx, float* gamma, int B, int Tmax,
    int K, int F, hipStream_t stream) {
    if (B <= 0) return;
    hipLaunchKernelGGL(hmm_estep_kernel,
                       dim3((B + HMM_WAVES - 1) / HMM_WAVES),
                       dim3(HMM_WAVES * WAVE), 0, stream, X, lengths, mu,
                       var, logA, logpi, alpha_ws, c_ws, ll, gamma0,
                       gamma_sum, gamma_head, xi_sum, sx, sxx, gamma, B,
                       Tmax, K, F);
}

extern "C" void launch_hmm_viterbi(
    const float* X, const int* lengths, const float* mu, const float* var,
    const float* logA, const float* logpi, unsigned char* bp_ws, int* path,
    int B, int Tmax, int K, int F, hipStream_t stream) {
    if (B <= 0) return;
    hipLaunchKernelGGL(hmm_viterbi_kernel,
                       dim3((B + HMM_WAVES - 1) / HMM_WAVES),
                       dim3(HMM_WAVES * WAVE), 0, stream, X, lengths, mu,
                       var, logA, logpi, bp_ws, path, B, Tmax, K, F);
}
