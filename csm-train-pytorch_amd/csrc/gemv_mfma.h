// The decode product at five to sixteen batch rows: ONE MFMA kernel and ONE launcher for both weight formats - bf16 [N][K]
// (generate.hip: csm_gemv_bf16*) and e4m3 [N][K] with an fp32 scale per row (quant.hip: csm_gemv_fp8w*).  The format is a template
// parameter (a policy struct below) that carries the five places where the two products differ and nothing else; every other
// line - the k ownership, the RMSNorm prologue, the wave-ordered reduction, the per-row K-extension, the epilogues - is shared, so
// FP8 mode decodes the bits of bf16 mode on the dequantised weights wherever the scales are powers of two by construction
// (tests/test_fp8_decode_gpu.py).  Everything here sits in the including file's anonymous namespace, like gemv_ext.h.
#pragma once
#include "common.h"
#include "gemv_ext.h"

namespace {

typedef float q_f2 __attribute__((ext_vector_type(2)));

// two e4m3 words (8 bytes) -> one bf16x8 MFMA fragment (exact: the fp32 image's low 16 bits are zero)
__device__ __forceinline__ bf16x8 cvt8_bf16(uint32_t a, uint32_t b) {
    const q_f2 a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, false), a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, true);
    const q_f2 b0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false), b1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, true);
    U4 u;
    u.x = (__float_as_uint(a0[0]) >> 16) | (__float_as_uint(a0[1]) & 0xffff0000u);
    u.y = (__float_as_uint(a1[0]) >> 16) | (__float_as_uint(a1[1]) & 0xffff0000u);
    u.z = (__float_as_uint(b0[0]) >> 16) | (__float_as_uint(b0[1]) & 0xffff0000u);
    u.w = (__float_as_uint(b1[0]) >> 16) | (__float_as_uint(b1[1]) & 0xffff0000u);
    return __builtin_bit_cast(bf16x8, u);
}

// ----------------------------------------------------------------------------------------------------- weight formats
// A format gives: the element type and the kernel's by-value weight argument; NL, the 16-byte loads that hold a lane's 16
// weights of a 64-k step; frag(loads, h), the weight fragment of the step's MFMA h (the lane's weights 8 h .. 8 h + 7);
// scaled(v, arg, n), what becomes of output row n's wave-ordered sum; sumsq, one step of the RMSNorm prologue's sum of squares;
// and for the launcher the K granularity, the entry point's name and the name csm_gemv_last_kernel() reports.
struct WeightBf16 {
    typedef bf16_t elem;
    struct Arg { const bf16_t* W; };
    static constexpr int NL = 2;                              // 32 bytes: the four lanes of a row fetch its whole 128-byte line
    static constexpr int KQ = 32;
    static constexpr const char* entry = "csm_gemv_bf16";
    static const char* kernel_name(int) { return "gemv_mfma_kernel<%d, %s, %d, %d, ext%d>"; }
    static __device__ __forceinline__ bf16x8 frag(const U4 (&q)[NL], int h) { return __builtin_bit_cast(bf16x8, q[h]); }
    static __device__ __forceinline__ float scaled(float v, const Arg&, int) { return v; }
    // The ONE place inside the kernel where the two formats round differently: here the square is rounded before it is added
    // (the compiler packs two multiplies into a v_pk_mul_f32), the FP8 format fuses.  Kept apart on purpose: making them alike
    // moves the last bit of rstd, and with it the decoded bits, of one of the two modes ('One MFMA kernel for both
    // weight formats').  So under the norm prologue FP8 == bf16 at power-of-two scales holds only where the sum is exact.
    static __device__ __forceinline__ float sumsq(float ss, float f) {
#pragma clang fp contract(off)
        return ss + f * f;
    }
};
struct WeightFp8 {
    typedef uint8_t elem;
    struct Arg { const uint8_t* W; const float* scale; };     // scale: [N] fp32, applied ONCE to the finished row sum
    static constexpr int NL = 1;                              // 16 bytes; bytes 0-7 and 8-15 are the fragments of the two MFMAs
    static constexpr int KQ = 16;
    static constexpr const char* entry = "csm_gemv_fp8w";
    static const char* kernel_name(int ek) { return ek ? "gemv_fp8_mfma_kernel<%d, %s, %d, %d, ext2>" : "gemv_fp8_mfma_kernel<%d, %s, %d, %d>"; }
    static __device__ __forceinline__ bf16x8 frag(const U4 (&q)[NL], int h) { return h ? cvt8_bf16(q[0].z, q[0].w) : cvt8_bf16(q[0].x, q[0].y); }
    static __device__ __forceinline__ float scaled(float v, const Arg& a, int n) { return v * a.scale[n]; }
    static __device__ __forceinline__ float sumsq(float ss, float f) { return __builtin_fmaf(f, f, ss); }   // (see WeightBf16::sumsq)
};

// ---------------------------------------------------------------------------------------------- five to sixteen batch rows
// The product as MFMA tiles, D[n][b] = sum_k W[n][k] x^[b][k] with v_mfma_f32_16x16x32_bf16, A = 16 weight rows, B = x^ transposed
// with the batch rows padded to 16 by zeros (never stored).  A workgroup owns one tile of 16 weight rows (8 gate/up pairs under
// SWIGLU) and its eight waves split K: wave w takes the 64-k steps s = w, w + 8, w + 16, ...  In a step lane l (column c = l & 15,
// k group g = l >> 4) loads the 16 contiguous weights of row n0 + c at k = 64 s + 16 g (WF::NL 16-byte loads; e4m3 weights are
// converted to bf16 in registers, exactly) and uses the first and the second eight as the fragments of two MFMAs.  The fragment's
// k order is thereby permuted (element j of group g is k = 16 g + j, resp. 16 g + 8 + j): the B fragment is loaded with the same
// permutation, x^[c][64 s + 16 g ..], straight from global memory (x is a few KB, L2 resident).  No LDS copy of x: every element
// of x^ is multiplied by exactly one wave of the workgroup, so staging it would add a round trip and a barrier and save nothing.
// Weights go global -> VGPRs, a segment of SEG steps in flight per lane before the first MFMA waits for them (non-temporal under NT).
// RMSNorm prologue: the workgroup's waves compute rstd of the batch rows in gemv_kernel's ORDER (lane-strided 8-element chunks,
// wave_sum; the rounding of each step is the format's, WF::sumsq) behind one barrier that keeps the weight loads in flight;
// x^ = bf16(x rstd w) as the B <= 4 kernels round it.
// The eight partial tiles meet in LDS and are summed in wave order 0..7 (no atomics), then WF::scaled.  Every output column sees
// only its own batch row's operands in an order fixed by K, so a row's result is the same bits for any B in 5..16, any position
// of the row in the batch and any contents of the other rows (tests/test_generate_wide_batch_gpu.py).  It is not bit-equal to the
// B <= 4 kernels, which sum in another order.
// Trailing pack (empty: the plain product, or one GemvExtRows): the epilogue thread of output (n, b) adds row b's own adapter's
// extension sum_j t[b][j] Bx[a_b][n][j] to the (scaled) sum, one fmaf per j in ascending j (then the adapter's bias), before
// the rounding / SwiGLU / residual epilogue.  It reads only row b's operands, so a row keeps its bits for any B in 5..16, any
// position and any batch-mates and their adapters; a row without adapter takes no extension: the plain product's bits.
// Every multiply-add of the body is written as what it is (contraction is off): no rounding is left to the compiler.
template <typename WF, int SEG, typename OutT, bool SWIGLU, bool NT, typename... Ext>
__global__ __launch_bounds__(512) void gemv_mfma_kernel(const bf16_t* __restrict__ x, const typename WF::Arg w, OutT* __restrict__ y,
                                                        const bf16_t* __restrict__ R, int B, int N, int K, int ldw, int ldx, int ldy,
                                                        const bf16_t* __restrict__ norm_w, float eps, const int* __restrict__ row_index,
                                                        int row_offset, Ext... ext) {
#pragma clang fp contract(off)
    constexpr int EK = ExtKind<Ext...>::v;
    static_assert(EK != 1, "gemv_mfma_kernel takes the per-row extension only");
    constexpr int NW = 8, NL = WF::NL;
    __shared__ float rs[16];
    __shared__ float part[NW][16][17];                        // [wave][weight row of the tile][batch row] (+1: no bank conflicts)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int n0 = blockIdx.x * 16;
    const int S = (K + 63) >> 6;                              // 64-k steps; the last one may be partial (K % 64 != 0: its first groups only)
    const typename WF::elem* wrow = w.W + (size_t)min(n0 + c, N - 1) * ldw + 16 * g;   // (rows past N re-read row N-1, never stored)
    const bool brow = c < B;
    const size_t xr = brow ? (row_index ? (size_t)(row_index[c] + row_offset) : (size_t)c) : (size_t)0;
    const bf16_t* xrow = x + xr * ldx + 16 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int nseg = (S + NW * SEG - 1) / (NW * SEG);
    for (int sg = 0; sg < nseg; ++sg) {
        U4 wq[SEG][NL], xq[SEG][2];
        const U4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const int s = (sg * SEG + i) * NW + wv;
            const int k = 64 * s + 16 * g;
#pragma unroll
            for (int l = 0; l < NL; ++l) wq[i][l] = z;
            if (s < S && k < K) {
                const U4* p = reinterpret_cast<const U4*>(wrow + 64 * s);
#pragma unroll
                for (int l = 0; l < NL; ++l) wq[i][l] = NT ? __builtin_nontemporal_load(p + l) : p[l];
            }
        }
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const int s = (sg * SEG + i) * NW + wv;
            const int k = 64 * s + 16 * g;
            xq[i][0] = z; xq[i][1] = z;
            if (brow && s < S && k < K) {
                const U4* p = reinterpret_cast<const U4*>(xrow + 64 * s);
                xq[i][0] = p[0]; xq[i][1] = p[1];
            }
        }
        if (norm_w) {
            if (sg == 0) {
                // rstd of batch rows wv, wv + 8 (gemv_kernel's summation order, the format's rounding); one barrier, LDS only: the
                // weights stay in flight
                for (int b = wv; b < B; b += NW) {
                    const bf16_t* xb = x + (row_index ? (size_t)(row_index[b] + row_offset) : (size_t)b) * ldx;
                    float ss = 0.f;
                    for (int q = lane; q < (K >> 3); q += 64) {
                        float f[8];
                        unpack8(*reinterpret_cast<const U4*>(xb + q * 8), f);
#pragma unroll
                        for (int j = 0; j < 8; ++j) ss = WF::sumsq(ss, f[j]);
                    }
                    ss = wave_sum(ss);
                    if (lane == 0) rs[b] = rsqrtf(ss / (float)K + eps);
                }
                lds_barrier();
            }
            if (brow) {
                const float r = rs[c];
#pragma unroll
                for (int i = 0; i < SEG; ++i) {
                    const int s = (sg * SEG + i) * NW + wv;
                    const int k = 64 * s + 16 * g;
                    if (s < S && k < K) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            float f[8], w8[8];
                            unpack8(xq[i][h], f);
                            unpack8(*reinterpret_cast<const U4*>(norm_w + k + 8 * h), w8);
#pragma unroll
                            for (int j = 0; j < 8; ++j) f[j] = f[j] * r * w8[j];
                            xq[i][h] = pack8(f);                      // the bf16 rounding of the B <= 4 kernels' x^
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const int s = (sg * SEG + i) * NW + wv;
            if (s < S) {                                              // (wave-uniform)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WF::frag(wq[i], 0), __builtin_bit_cast(bf16x8, xq[i][0]), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WF::frag(wq[i], 1), __builtin_bit_cast(bf16x8, xq[i][1]), acc, 0, 0, 0);
            }
        }
    }
    // lane holds D[weight row 4 g + r][batch row c]; the eight K slices are added in wave order
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wv][4 * g + r][c] = acc[r];
    __syncthreads();
    const int t = threadIdx.x;
    if constexpr (SWIGLU) {
        const int i = t & 7, b = t >> 3;                      // output n0 / 2 + i of batch row b: gate row 2 i, up row 2 i + 1
        if (b < B && n0 + 2 * i < N) {
            float gs = part[0][2 * i][b], us = part[0][2 * i + 1][b];
#pragma unroll
            for (int wi = 1; wi < NW; ++wi) { gs += part[wi][2 * i][b]; us += part[wi][2 * i + 1][b]; }
            gs = WF::scaled(gs, w, n0 + 2 * i);
            us = WF::scaled(us, w, n0 + 2 * i + 1);
            if constexpr (EK == 2) {
                const GemvExtRows& e = ext_rows_arg(ext...);
                const int a = ext_row_adapter(e, b);
                if (a >= 0) {
                    gs = ext_dot(gs, e.Bx[a] + (size_t)(n0 + 2 * i) * e.ldb, e.t + (size_t)b * e.ldt, e.kx);
                    us = ext_dot(us, e.Bx[a] + (size_t)(n0 + 2 * i + 1) * e.ldb, e.t + (size_t)b * e.ldt, e.kx);
                    gs += ext_row_bias(e, a, n0 + 2 * i);
                    us += ext_row_bias(e, a, n0 + 2 * i + 1);
                }
            }
            const float gg = bf2f(f2bf(gs)), u = bf2f(f2bf(us));
            float v = silu(gg) * u;
            const int n = (n0 >> 1) + i;
            if (R) v += bf2f(R[(size_t)b * ldy + n]);
            y[(size_t)b * ldy + n] = f2bf(v);
        }
    } else {
        const int rr = t & 15, b = t >> 4;
        const int n = n0 + rr;
        if (b < B && n < N) {
            float v = part[0][rr][b];
#pragma unroll
            for (int wi = 1; wi < NW; ++wi) v += part[wi][rr][b];
            v = WF::scaled(v, w, n);
            if constexpr (EK == 2) {
                const GemvExtRows& e = ext_rows_arg(ext...);
                const int a = ext_row_adapter(e, b);
                if (a >= 0) v = ext_dot(v, e.Bx[a] + (size_t)n * e.ldb, e.t + (size_t)b * e.ldt, e.kx) + ext_row_bias(e, a, n);
            }
            if (R) v += bf2f(R[(size_t)b * ldy + n]);
            if constexpr (sizeof(OutT) == 2) y[(size_t)b * ldy + n] = f2bf(v);
            else y[(size_t)b * ldy + n] = v;
        }
    }
}

// B = 5..16: one workgroup per 16 weight rows; SEG = 64-k steps per wave and segment, sized so that K <= 2048 runs as one segment
// (K = 8192: two of eight steps).  The caller has checked its entry point's arguments and decides nt (non-temporal weight loads).
// ext: empty or one GemvExtRows, the kernel's trailing pack.
template <typename WF, typename... Ext>
static int gemv_mfma_launch(typename WF::Arg w, const void* x, void* y, const void* residual, int B, int N, int K, int ldw, int ldx,
                            int ldy, int out_f32, const void* norm_w, float eps, int swiglu, const int* row_index, int row_offset,
                            bool nt, hipStream_t stream, Ext... ext) {
    if constexpr (WF::KQ == 32) CSM_REQUIRE((K & 31) == 0, "csm_gemv_bf16: B=%d needs K %% 32 == 0 (K=%d)", B, K);
    const int grid = (N + 15) / 16;
    const int spw = ((K + 63) / 64 + 7) / 8;                  // 64-k steps per wave
    const int seg = spw <= 1 ? 1 : (spw <= 2 ? 2 : (spw <= 4 ? 4 : 8));
#define LM(SEG, T, SW, NT_) hipLaunchKernelGGL((gemv_mfma_kernel<WF, SEG, T, SW, NT_, Ext...>), dim3(grid), dim3(512), 0, stream, (const bf16_t*)x, w, (T*)y, (const bf16_t*)residual, B, N, K, ldw, ldx, ldy, (const bf16_t*)norm_w, eps, row_index, row_offset, ext...)
#define LMS(T, SW, NT_) do { if (seg == 1) LM(1, T, SW, NT_); else if (seg == 2) LM(2, T, SW, NT_); else if (seg == 4) LM(4, T, SW, NT_); else LM(8, T, SW, NT_); } while (0)
    if (swiglu) { if (nt) LMS(bf16_t, true, true); else LMS(bf16_t, true, false); }
    else if (out_f32) { if (nt) LMS(float, false, true); else LMS(float, false, false); }
    else { if (nt) LMS(bf16_t, false, true); else LMS(bf16_t, false, false); }
#undef LMS
#undef LM
    g_last_gemv = {WF::kernel_name(ExtKind<Ext...>::v), (out_f32 && !swiglu) ? "float" : "bf16",
                   {seg, swiglu ? 1 : 0, nt ? 1 : 0, ExtKind<Ext...>::v, 0, 0}};
    CSM_CHECK_LAUNCH(WF::entry);
    return 0;
}

}  // namespace
