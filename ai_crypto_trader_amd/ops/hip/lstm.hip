// Fused LSTM sequence kernels (BASELINE config #2).
//
// Replaces neural_network_service.py's Keras LSTM stack (:164-421) with a
// hand-written gfx950 recurrent cell: ONE kernel launch marches the whole
// sequence, W_hh stays resident in LDS, h feeds back through LDS, and the
// per-step gate GEMM (batch-tile 64 x 4H x H) runs on
// v_mfma_f32_16x16x32_bf16 with the input projection (x @ W_ih, a plain
// hipBLASLt GEMM on the torch side) pre-computed and read as the
// accumulator init. No Triton, no CUDA shims, no per-step launches.
//
// Tile decomposition, fragment mapping, LDS staging, activations and the
// guarded launch are the shared recurrent tile core (rnn_tile.hpp), here
// with the four gates i,f,g,o: a lane holds all four for the same (row, n),
// so c = f*c + i*g, h = o*tanh(c) is register-local and c lives in
// registers across the whole sequence.
//
// Backward: reverse-time kernel computes the sequential part only
// (per-step dgates + the dh_rec = dgates @ W_hh^T chain). The big
// batched reductions dW_hh = sum_t h_{t-1}^T dgates_t, dW_ih, db are
// single hipBLASLt GEMMs on the torch side (models/lstm.py).

#include "rnn_tile.hpp"

namespace {

// MULTI adds the model axis: blockIdx.y = model over model-major slabs,
// each exactly the single-model layout. The single-model launchers keep
// the MULTI = false instantiations, whose code has no model arithmetic.
template <int H, bool MULTI>
__global__ void __launch_bounds__((H / 16) * 64) lstm_seq_fwd_kernel(
    const bf16* __restrict__ xproj,    // (M, T, B, 4H) x@W_ih + b_ih (bf16)
    const bf16* __restrict__ Wt,       // (M, 4H, H)  W_hh transposed, n-major
    const float* __restrict__ bias,    // (M, 4H)     b_hh
    bf16* __restrict__ h_out,          // (M, T, B, H)
    bf16* __restrict__ gates_out,      // (M, T, B, 4H) post-activation i,f,g,o
    float* __restrict__ c_out,         // (M, T, B, H)
    int B, int T, int save_mode)       // 0: inference (h only), 1: training
{
    constexpr int NT = (H / 16) * 64;   // threads per block
    constexpr int FOURH = 4 * H;
    constexpr int HP = H + RNN_PAD;

    __shared__ bf16 lds_h[RNN_BM * HP];
    __shared__ bf16 lds_w[FOURH * HP];

    const int b0 = blockIdx.x * RNN_BM;
    const RnnLane ln = rnn_lane();
    const int fq = ln.fq;
    if constexpr (MULTI) {
        // per-model bases, 64-bit and wave-uniform: the per-lane index
        // math below is the single-model one
        const long model = blockIdx.y;
        const long model_tb = model * T * B;   // row offset of this slab
        xproj += model_tb * FOURH;
        h_out += model_tb * H;
        if (save_mode) {                       // null in inference mode
            gates_out += model_tb * FOURH;
            c_out += model_tb * H;
        }
        Wt += model * (FOURH * H);
        bias += model * FOURH;
    }

    rnn_stage<FOURH, H, NT>(lds_w, Wt);     // W_hh^T (4H x H)
    rnn_zero_h<H, NT>(lds_h);
    __syncthreads();

    const int ncol = ln.ncol();
    float bias_g[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias_g[g] = bias[g * H + ncol];

    float c_reg[RNN_MT][4];            // [m_tile][reg] cell state
#pragma unroll
    for (int mt = 0; mt < RNN_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) c_reg[mt][r] = 0.0f;

    for (int t = 0; t < T; ++t) {
        // ---- gates = h @ W_hh^T(+) xproj + bias --------------------------
        f32x4 acc[RNN_MT][4];          // [m_tile][gate]
        const long base_tb = ((long)t * B + b0);
#pragma unroll
        for (int mt = 0; mt < RNN_MT; ++mt) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = g * H + ncol;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = mt * 16 + fq * 4 + r;
                    acc[mt][g][r] =
                        (float)xproj[(base_tb + row) * FOURH + col] +
                        bias_g[g];
                }
            }
        }
#pragma unroll
        for (int ks = 0; ks < H / 32; ++ks) {
            const int k0 = ks * 32 + fq * 8;
#pragma unroll
            for (int mt = 0; mt < RNN_MT; ++mt) {
                const int arow = mt * 16 + ln.fr;
                bf16x8 a = *reinterpret_cast<const bf16x8*>(
                    &lds_h[arow * HP + k0]);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int bcol = g * H + ncol;
                    bf16x8 b = *reinterpret_cast<const bf16x8*>(
                        &lds_w[bcol * HP + k0]);
                    acc[mt][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a, b, acc[mt][g], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // all reads of lds_h done before overwrite

        // ---- cell update + write h ---------------------------------------
#pragma unroll
        for (int mt = 0; mt < RNN_MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + fq * 4 + r;
                const float gi = rnn_sigmoid(acc[mt][0][r]);
                const float gf = rnn_sigmoid(acc[mt][1][r]);
                const float gg = rnn_tanh(acc[mt][2][r]);
                const float go = rnn_sigmoid(acc[mt][3][r]);
                const float c = gf * c_reg[mt][r] + gi * gg;
                c_reg[mt][r] = c;
                const float h = go * rnn_tanh(c);
                const bf16 hb = (bf16)h;
                lds_h[row * HP + ncol] = hb;
                if (save_mode) {       // backward saves: ~5x the stores of
                                       // the inference path, skip them there
                    const long gb = (base_tb + row) * FOURH;
                    gates_out[gb + 0 * H + ncol] = (bf16)gi;
                    gates_out[gb + 1 * H + ncol] = (bf16)gf;
                    gates_out[gb + 2 * H + ncol] = (bf16)gg;
                    gates_out[gb + 3 * H + ncol] = (bf16)go;
                    c_out[(base_tb + row) * H + ncol] = c;
                }
                h_out[(base_tb + row) * H + ncol] = hb;
            }
        }
        __syncthreads();
    }
}

template <int H, bool MULTI>
__global__ void __launch_bounds__((H / 16) * 64) lstm_seq_bwd_kernel(
    const float* __restrict__ dh_up,   // (M, T, B, H) upstream grad
    const bf16* __restrict__ gates,    // (M, T, B, 4H) saved i,f,g,o
    const float* __restrict__ c_sav,   // (M, T, B, H)
    const bf16* __restrict__ W,        // (M, H, 4H)  W_hh row-major
    bf16* __restrict__ dgates_out,     // (M, T, B, 4H)
    int B, int T)
{
    constexpr int NT = (H / 16) * 64;
    constexpr int FOURH = 4 * H;
    constexpr int GP = FOURH + RNN_PAD;

    __shared__ bf16 lds_dg[RNN_BM * GP];    // dgates tile (A operand)
    __shared__ bf16 lds_w[H * GP];          // W_hh (B operand: k=4H contig)

    const int b0 = blockIdx.x * RNN_BM;
    const RnnLane ln = rnn_lane();
    const int fq = ln.fq;
    if constexpr (MULTI) {                // as in the forward kernel
        const long model = blockIdx.y;
        const long model_tb = model * T * B;
        dh_up += model_tb * H;
        gates += model_tb * FOURH;
        c_sav += model_tb * H;
        dgates_out += model_tb * FOURH;
        W += model * (H * FOURH);
    }

    rnn_stage<H, FOURH, NT>(lds_w, W);
    __syncthreads();

    const int ncol = ln.ncol();
    float dc[RNN_MT][4];
    float dhrec[RNN_MT][4];
#pragma unroll
    for (int mt = 0; mt < RNN_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { dc[mt][r] = 0.0f; dhrec[mt][r] = 0.0f; }

    for (int t = T - 1; t >= 0; --t) {
        const long base_tb = ((long)t * B + b0);
#pragma unroll
        for (int mt = 0; mt < RNN_MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + fq * 4 + r;
                const long gb = (base_tb + row) * FOURH;
                const float gi = (float)gates[gb + 0 * H + ncol];
                const float gf = (float)gates[gb + 1 * H + ncol];
                const float gg = (float)gates[gb + 2 * H + ncol];
                const float go = (float)gates[gb + 3 * H + ncol];
                const float c = c_sav[(base_tb + row) * H + ncol];
                const float cprev =
                    (t > 0) ? c_sav[((base_tb - B) + row) * H + ncol] : 0.0f;
                const float tc = rnn_tanh(c);
                const float dh =
                    dh_up[(base_tb + row) * H + ncol] + dhrec[mt][r];
                const float do_ = dh * tc;
                float dcv = dc[mt][r] + dh * go * (1.0f - tc * tc);
                const float di = dcv * gg;
                const float df = dcv * cprev;
                const float dgg = dcv * gi;
                dc[mt][r] = dcv * gf;               // dc_{t-1}
                const float dai = di * gi * (1.0f - gi);
                const float daf = df * gf * (1.0f - gf);
                const float dag = dgg * (1.0f - gg * gg);
                const float dao = do_ * go * (1.0f - go);
                const bf16 b_i = (bf16)dai, b_f = (bf16)daf;
                const bf16 b_g = (bf16)dag, b_o = (bf16)dao;
                lds_dg[row * GP + 0 * H + ncol] = b_i;
                lds_dg[row * GP + 1 * H + ncol] = b_f;
                lds_dg[row * GP + 2 * H + ncol] = b_g;
                lds_dg[row * GP + 3 * H + ncol] = b_o;
                dgates_out[gb + 0 * H + ncol] = b_i;
                dgates_out[gb + 1 * H + ncol] = b_f;
                dgates_out[gb + 2 * H + ncol] = b_g;
                dgates_out[gb + 3 * H + ncol] = b_o;
            }
        }
        __syncthreads();

        // dh_rec = dgates @ W_hh^T : (BM x 4H) @ (4H x H) -> (BM x H)
        f32x4 acc[RNN_MT];
#pragma unroll
        for (int mt = 0; mt < RNN_MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int ks = 0; ks < FOURH / 32; ++ks) {
            const int k0 = ks * 32 + fq * 8;
#pragma unroll
            for (int mt = 0; mt < RNN_MT; ++mt) {
                const int arow = mt * 16 + ln.fr;
                bf16x8 a = *reinterpret_cast<const bf16x8*>(
                    &lds_dg[arow * GP + k0]);
                // B[k][n] = W_hh[n][k]: row n of W, 8 contiguous k
                bf16x8 b = *reinterpret_cast<const bf16x8*>(
                    &lds_w[ncol * GP + k0]);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a, b, acc[mt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < RNN_MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) dhrec[mt][r] = acc[mt][r];
        __syncthreads();
    }
}

// --- bf16 MFMA layout validation GEMM: C = A @ B, f32 out ----------------
__global__ void mfma_gemm_test_bf16_kernel(const bf16* __restrict__ A,
                                           const bf16* __restrict__ B,
                                           float* __restrict__ C, int M,
                                           int N, int K) {
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 16;
    const int lane = threadIdx.x & 63;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 32) {
        bf16x8 a, b;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a[j] = A[(long)(i0 + (lane & 15)) * K + k0 + 8 * (lane >> 4) + j];
            b[j] = B[(long)(k0 + 8 * (lane >> 4) + j) * N + j0 + (lane & 15)];
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        C[(long)(i0 + (lane >> 4) * 4 + r) * N + j0 + (lane & 15)] = acc[r];
}

}  // namespace

// Shared launchers: grid = (B/64 batch tiles, M models). The single-model
// entry points launch the MULTI = false instantiations with M = 1.
template <bool MULTI>
static void lstm_fwd_launch(const char* who, const void* xproj,
                            const void* Wt, const float* bias, void* h_out,
                            void* gates_out, float* c_out, int M, int B,
                            int T, int H, int save_mode,
                            hipStream_t stream) {
    rnn_launch(who, lstm_seq_fwd_kernel<64, MULTI>,
               lstm_seq_fwd_kernel<32, MULTI>, M, B, H, stream,
               (const bf16*)xproj, (const bf16*)Wt, bias, (bf16*)h_out,
               (bf16*)gates_out, c_out, B, T, save_mode);
}

template <bool MULTI>
static void lstm_bwd_launch(const char* who, const float* dh_up,
                            const void* gates, const float* c_sav,
                            const void* W, void* dgates_out, int M, int B,
                            int T, int H, hipStream_t stream) {
    rnn_launch(who, lstm_seq_bwd_kernel<64, MULTI>,
               lstm_seq_bwd_kernel<32, MULTI>, M, B, H, stream, dh_up,
               (const bf16*)gates, c_sav, (const bf16*)W, (bf16*)dgates_out,
               B, T);
}

extern "C" void launch_lstm_seq_fwd(const void* xproj, const void* Wt,
                                    const float* bias, void* h_out,
                                    void* gates_out, float* c_out, int B,
                                    int T, int H, int save_mode,
                                    hipStream_t stream) {
    lstm_fwd_launch<false>("lstm_fwd", xproj, Wt, bias, h_out, gates_out,
                           c_out, 1, B, T, H, save_mode, stream);
}

extern "C" void launch_lstm_seq_bwd(const float* dh_up, const void* gates,
                                    const float* c_sav, const void* W,
                                    void* dgates_out, int B, int T, int H,
                                    hipStream_t stream) {
    lstm_bwd_launch<false>("lstm_bwd", dh_up, gates, c_sav, W, dgates_out,
                           1, B, T, H, stream);
}

// M independent models in one launch; every array is model-major.
extern "C" void launch_lstm_seq_fwd_multi(const void* xproj, const void* Wt,
                                          const float* bias, void* h_out,
                                          void* gates_out, float* c_out,
                                          int M, int B, int T, int H,
                                          int save_mode,
                                          hipStream_t stream) {
    lstm_fwd_launch<true>("lstm_fwd_multi", xproj, Wt, bias, h_out,
                          gates_out, c_out, M, B, T, H, save_mode, stream);
}

extern "C" void launch_lstm_seq_bwd_multi(const float* dh_up,
                                          const void* gates,
                                          const float* c_sav, const void* W,
                                          void* dgates_out, int M, int B,
                                          int T, int H, hipStream_t stream) {
    lstm_bwd_launch<true>("lstm_bwd_multi", dh_up, gates, c_sav, W,
                          dgates_out, M, B, T, H, stream);
}

extern "C" void launch_mfma_gemm_test_bf16(const void* A, const void* B,
                                           float* C, int M, int N, int K,
                                           hipStream_t stream) {
    dim3 grid(M / 16, N / 16);
    hipLaunchKernelGGL(mfma_gemm_test_bf16_kernel, grid, dim3(64), 0, stream,
                       (const bf16*)A, (const bf16*)B, C, M, N, K);
}
