// Recurrent tile core shared by lstm.hip and gru.hip (G = 4 / 3 gates).
//
// Decomposition (template H, NW = H/16 waves per block):
//   block = 64-row batch tile; wave w owns hidden columns [16w, 16w+16)
//   ACROSS all G gates, so a lane holds every gate of the same (row, n) and
//   the cell update is register-local. W_hh stays resident in LDS for the
//   whole sequence and h round-trips LDS (padded stride -> conflict-free
//   b128 fragment reads); the per-step GEMMs run on
//   v_mfma_f32_16x16x32_bf16.
//
// Fragment mapping mfma_f32_16x16x32_bf16 (validated on-device by
// mfma_gemm_test_bf16 vs torch.matmul):
//   A[m][k]: lane l holds A[l&15][8*(l>>4) + j], j=0..7  (one b128 read)
//   B[k][n]: lane l holds B[8*(l>>4)+j][l&15]  -> store B n-major so the
//            8 k-elements are contiguous per lane
//   C[m][n]: lane l, reg r -> m = (l>>4)*4 + r, n = l&15
//
// The gate math (cell update, backward, save-mode stores) is per cell and
// stays in the two .hip files. So do the two per-step MFMA loop nests:
// as inlined functions they compile to a different load order in the time
// loop (lstm_seq_fwd_kernel<32>: 268 -> 296 us at B = 16384, T = 60),
// written in the kernels the time loops are instruction-identical.
#pragma once

#include <stdexcept>
#include <string>

#include "common.hpp"

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RNN_MT = 4;             // M-tiles per wave
constexpr int RNN_BM = 16 * RNN_MT;   // 64-row batch tiles: B/64 blocks per
                                      // model (1 block/CU at B=16384)
constexpr int RNN_PAD = 8;            // LDS row padding, bf16 (bank-spread)

// 1-ulp v_rcp instead of IEEE div: the gate math is tolerance-tested
// against PyTorch fp32 (not bitwise), and libm-grade division costs
// ~10 instrs per gate element per timestep.
DEV_INLINE float rnn_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
DEV_INLINE float rnn_tanh(float x) {
    // tanh(x) = 2*sigmoid(2x) - 1, rcp as above
    return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f;
}

struct RnnLane {
    int w;      // wave id = hidden sub-column
    int fr;     // fragment col
    int fq;     // fragment row group / k group
    DEV_INLINE int ncol() const { return 16 * w + fr; }   // hidden column
};
DEV_INLINE RnnLane rnn_lane() {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    return {tid >> 6, lane & 15, lane >> 4};
}

// Stage a row-major ROWS x COLS matrix into LDS with row stride
// COLS + RNN_PAD: W_hh^T (G*H x H) forward, W_hh (H x G*H) backward.
template <int ROWS, int COLS, int NT>
DEV_INLINE void rnn_stage(bf16 (&lds)[ROWS * (COLS + RNN_PAD)],
                          const bf16* src) {
    for (int i = threadIdx.x; i < ROWS * COLS; i += NT)
        lds[(i / COLS) * (COLS + RNN_PAD) + (i % COLS)] = src[i];
}

template <int H, int NT>
DEV_INLINE void rnn_zero_h(bf16 (&lds_h)[RNN_BM * (H + RNN_PAD)]) {
    for (int i = threadIdx.x; i < RNN_BM * (H + RNN_PAD); i += NT)
        lds_h[i] = (bf16)0.0f;
}

// Guarded launch of the H = 64 / H = 32 instantiation of one kernel on a
// (B/64 batch tiles, M models) grid, H/16 waves per block. Throws before
// anything is launched.
template <typename K, typename... Args>
inline void rnn_launch(const char* who, K k64, K k32, int M, int B, int H,
                       hipStream_t stream, Args... args) {
    if (B <= 0 || B % RNN_BM != 0)
        throw std::runtime_error(std::string(who) +
                                 ": B must be a positive multiple of 64");
    if (M < 1 || M > 65535)
        throw std::runtime_error(std::string(who) +
                                 ": M must be in [1, 65535]");
    if (H != 64 && H != 32)
        throw std::runtime_error(std::string(who) + ": H must be 32 or 64");
    hipLaunchKernelGGL(H == 64 ? k64 : k32, dim3(B / RNN_BM, M),
                       dim3(H * 4), 0, stream, args...);
}
