// Weight-only FP8 decode (round 7): the one-position products of both stacks with OCP e4m3 weights and one fp32 scale per
// output row - csm_quantize_rows_fp8 makes them, csm_gemv_fp8w multiplies with them.  Activations stay bf16, products and sums
// are fp32, the scale is applied ONCE to the finished row sum:  y[b][n] = epilogue(scale[n] * sum_k x^[b][k] q[n][k]).
// e4m3 -> fp32 / bf16 is exact (v_cvt_pk_f32_fp8; a value has four significant bits), so the only rounding the mode adds is
// the quantiser's.  B <= 4: gemv_fp8_kernel below mirrors the bf16 families of generate.hip (gemv_reg_kernel / gemv_regn_kernel)
// with the weight operand replaced: weights global -> VGPRs in 16-byte loads (16 weights each), no LDS for them, fixed
// reduction order, no atomics.  B = 5..16 is no mirror: gemv_mfma.h's one kernel, instantiated with the e4m3 weight format.
//
// Per-row K-extension (csm_gemv_fp8w_kext_rows: an un-merged LoRA adapter per batch row on the quantised base; the packs and the
// extension's operations are gemv_ext.h's, shared with the bf16 families).  Row b with adapter a = row_adapter[b]:
//     y[b][n] = epilogue(scale[n] * sum_k x^[b][k] q[n][k]  +  sum_j t[b][j] Bx[a][n][j]  +  bias[a][n])
//   1. base = scale[n] * (the row sum), formed exactly as csm_gemv_fp8w forms it: same products, same order, ONE scaling of the
//      finished sum.  The scale belongs to the quantised weights alone - t and Bx are bf16 numbers that never saw the quantiser -
//      so the extension is NOT scaled.
//   2. ext = sum_j t[b][j] Bx[a][n][j] in fp32, a fixed order, starting from zero (VALU) or accumulated onto base (MFMA):
//        B <= 4 (gemv_fp8_kernel):       lane l owns extension chunk l (ext_load), ext_fma from 0 over its 8 elements in ascending
//                                        j, then a SECOND butterfly of the kernel's own shape (wave_sum; under SwiGLU the same
//                                        permlane32_swap pairing: gate partials to lanes 0-31, up partials to lanes 32-63, one
//                                        butterfly for both); v = base + ext.  The base butterfly is untouched: the lane partials
//                                        of the main loop are never mixed with extension terms.
//        B = 5..16 (gemv_mfma_kernel):   the epilogue thread of output (n, b) runs ext_dot ONTO base, one fmaf per j in
//                                        ascending j, as the bf16 instantiation does onto its un-scaled sum.
//   3. v += bias[a][n] (0 where the table or the adapter's entry is NULL), then the existing epilogue: SwiGLU rounds gate and up to
//      bf16 after extension and bias; residual; bf16 or fp32 store.
// A row with a = -1 or a >= n_adapters skips 2 and 3 altogether (a wave-uniform branch, not an addition of zero): the bits of
// csm_gemv_fp8w at the same B.  Every step reads row b's operands only and the VALU steps are the same operations for every NB,
// so the plain kernels' two promises carry over: B <= 4, row b of a B-row launch is the one-row launch's bits; B = 5..16, a row's
// bits do not depend on B, its position or its batch-mates and their adapters.  No atomics.  The plain instantiations have an
// empty pack: their signature, code and bits are what they were.
#include "common.h"
#include "gemv_ext.h"
#include "gemv_mfma.h"
#include <math.h>

// Every multiply-add below is written out (__builtin_fmaf / elementwise_fma): nothing is left to the compiler's contraction, which
// may differ between two inlined copies of one expression - the one-row and the B-row kernels must agree bit for bit.
#pragma clang fp contract(off)

namespace {

// 16 e4m3 bytes -> 16 fp32 (exact), in byte order  (q_f2 and cvt8_bf16, the MFMA fragment's conversion: gemv_mfma.h)
__device__ __forceinline__ void cvt16(const U4& q, float* f) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const q_f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[w], false);
        const q_f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[w], true);
        f[4 * w] = lo[0]; f[4 * w + 1] = lo[1]; f[4 * w + 2] = hi[0]; f[4 * w + 3] = hi[1];
    }
}

// ------------------------------------------------------------------------------------------------------------- quantiser
// One wave per row: amax = max |w|, scale = amax / 448 (a true, correctly rounded fp32 division; 1 for an all-zero row),
// q = e4m3fn(clamp(w / scale, -448, 448)) with round-to-nearest-even - the clamp makes the conversion saturating, so no NaN code
// can come out of finite weights.  csm/quant.py restates the rule in torch; the two agree bit for bit.
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const bf16_t* __restrict__ W, uint8_t* __restrict__ W8,
                                                                float* __restrict__ scale, int N, int K, int ldw, int ldw8) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    const bf16_t* w = W + (size_t)n * ldw;
    float amax = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        float f[8];
        unpack8(*reinterpret_cast<const U4*>(w + k), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
    }
    amax = wave_max(amax);
    const float s = amax > 0.f ? amax / 448.f : 1.f;
    if (lane == 0) scale[n] = s;
    uint8_t* q = W8 + (size_t)n * ldw8;
    for (int k = lane * 8; k < K; k += 512) {
        float f[8];
        unpack8(*reinterpret_cast<const U4*>(w + k), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(f[j] / s, -448.f), 448.f);
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        *reinterpret_cast<uint2*>(q + k) = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
}

// ---------------------------------------------------------------------------------------------- one to four batch rows
// Lane l owns, in chunk c < KC, the 16 elements k = 16 l + 1024 c .. + 15 (one 16-byte weight load; elements at k >= K are
// zeros on both sides).  A row of x in that ownership: two 16-byte bf16 loads per chunk.
template <int KC>
__device__ __forceinline__ void load_x16(const bf16_t* __restrict__ xrow, int K, int lane, U4 (&xr)[KC][2]) {
    const U4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        const int k = 16 * lane + 1024 * c;
        xr[c][0] = z; xr[c][1] = z;
        if (k < K) {
            const U4* p = reinterpret_cast<const U4*>(xrow + k);
            xr[c][0] = p[0]; xr[c][1] = p[1];
        }
    }
}
// rstd of the row (RMSNorm): squares added in the lane's element order, then the wave butterfly
template <int KC>
__device__ __forceinline__ float rstd16(const U4 (&xr)[KC][2], int K, float eps) {
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float f[8];
            unpack8(xr[c][h], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(f[j], f[j], ss);
        }
    ss = wave_sum(ss);
    return rsqrtf(ss / (float)K + eps);
}
// the lane's 16 elements of chunk c as fp32: x itself, or x^ = bf16(x rstd w) as the bf16 kernels round it
__device__ __forceinline__ void xhat16(const U4 (&xr)[2], const bf16_t* __restrict__ nw, float rs, float* f) {
    unpack8(xr[0], f);
    unpack8(xr[1], f + 8);
    if (nw) {
        float w8[16];
        unpack8(*reinterpret_cast<const U4*>(nw), w8);
        unpack8(*reinterpret_cast<const U4*>(nw + 8), w8 + 8);
#pragma unroll
        for (int j = 0; j < 16; ++j) f[j] = bf2f(f2bf(f[j] * rs * w8[j]));
    }
}

// y[b][n] = epilogue(scale[n] * sum_k x^[b][k] q[n][k]);  one wave per output (a gate / up pair under SWIGLU), NB <= 4 batch rows
// share every weight load.  NB == 1 (the mirror of gemv_reg_kernel): every wave holds x in registers, RMSNorm is a wave
// reduction, no LDS, no barrier, the weight rows are requested first.  NB = 2..4 (the mirror of gemv_regn_kernel): wave b prepares
// row b and publishes x^ as fp32 behind ONE barrier that leaves the weight loads in flight; a converted weight then feeds NB fused
// multiply-adds, two rows per v_pk_fma_f32.  Either way accumulator (row, output) sees fmaf(w_j, x^_j, acc) over the lane's
// elements in ascending k and then the same butterfly: row b of a B-row launch is bit-identical to the one-row launch.
// Fusions as csm_gemv_bf16_ex: norm_w (RMSNorm prologue), SWIGLU (interleaved gate / up rows, each scaled and rounded to bf16
// first), R (residual), fp32 output, row_index (x gathered from a table), NT (non-temporal weight loads).
template <int KC, int NB, typename OutT, bool SWIGLU, bool NT, typename... Ext>
__global__ __launch_bounds__(256) void gemv_fp8_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ W8,
                                                       const float* __restrict__ scale, OutT* __restrict__ y,
                                                       const bf16_t* __restrict__ R, int N, int K, int ldw8, int ldx, int ldy,
                                                       const bf16_t* __restrict__ norm_w, float eps, const int* __restrict__ row_index,
                                                       int row_offset, Ext... ext) {
    constexpr int EK = ExtKind<Ext...>::v;
    static_assert(EK != 1, "gemv_fp8_kernel takes the per-row extension only");
    constexpr int RW = SWIGLU ? 2 : 1;
    constexpr int NP = (NB + 1) / 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.x * (blockDim.x >> 6) + wv;
    const int NO = N / RW;
    const bool live = n < NO;                                   // (outputs past the end re-read the last rows, never stored)
    const int nn = live ? n : NO - 1;
    U4 wq[RW][KC];
    {
        const U4 z = {0u, 0u, 0u, 0u};
        const uint8_t* w = W8 + (size_t)nn * RW * ldw8 + 16 * lane;
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                wq[r][c] = z;
                if (16 * lane + 1024 * c < K) {
                    const U4* p = reinterpret_cast<const U4*>(w + (size_t)r * ldw8 + 1024 * c);
                    wq[r][c] = NT ? __builtin_nontemporal_load(p) : *p;
                }
            }
    }
    // GemvExtRows: row b's adapter (wave-uniform), its chunk of t and of the adapter's Bx rows, the adapter's bias.  Requested
    // beside the weights where the registers allow it (KC <= 2), after the main loop otherwise (K = 8192: a long loop, the
    // latency is small against it).
    [[maybe_unused]] int ea[NB];
    [[maybe_unused]] U4 et[NB], eb[RW][NB];
    [[maybe_unused]] float ebias[RW][NB];
    [[maybe_unused]] auto ext_fetch = [&]() {
        if constexpr (EK == 2) {
            const GemvExtRows& e = ext_rows_arg(ext...);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                ea[b] = __builtin_amdgcn_readfirstlane(ext_row_adapter(e, b));
                if (ea[b] >= 0) {
                    et[b] = ext_load(e.t + (size_t)b * e.ldt, lane, e.kx);
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
                        eb[r][b] = ext_load(e.Bx[ea[b]] + (size_t)(nn * RW + r) * e.ldb, lane, e.kx);
                        ebias[r][b] = ext_row_bias(e, ea[b], nn * RW + r);
                    }
                }
            }
        }
    };
    if constexpr (EK == 2 && KC <= 2) ext_fetch();
    q_f2 acc[RW][NP];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int q = 0; q < NP; ++q) acc[r][q] = (q_f2){0.f, 0.f};
    if constexpr (NB == 1) {
        if (!live) return;
        const size_t row = row_index ? (size_t)(row_index[0] + row_offset) : (size_t)0;
        U4 xr[KC][2];
        load_x16<KC>(x + row * ldx, K, lane, xr);
        const float rs = norm_w ? rstd16<KC>(xr, K, eps) : 1.f;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            float xf[16];
            xhat16(xr[c], (norm_w && 16 * lane + 1024 * c < K) ? norm_w + 16 * lane + 1024 * c : nullptr, rs, xf);
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                float wf[16];
                cvt16(wq[r][c], wf);
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[r][0].x = __builtin_fmaf(wf[j], xf[j], acc[r][0].x);
            }
            if constexpr (KC > 2) __builtin_amdgcn_sched_barrier(0);   // (K = 8192: one chunk's fp32 images live at a time - registers)
        }
    } else {
        extern __shared__ __attribute__((aligned(16))) char smem_q[];
        float (*xsh)[KC * 1024] = reinterpret_cast<float (*)[KC * 1024]>(smem_q);     // [NB][KC * 1024]
        if (wv < NB) {
            const size_t row = row_index ? (size_t)(row_index[wv] + row_offset) : (size_t)wv;
            U4 xr[KC][2];
            load_x16<KC>(x + row * ldx, K, lane, xr);
            const float rs = norm_w ? rstd16<KC>(xr, K, eps) : 1.f;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                float xf[16];
                xhat16(xr[c], (norm_w && 16 * lane + 1024 * c < K) ? norm_w + 16 * lane + 1024 * c : nullptr, rs, xf);
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    *reinterpret_cast<float4*>(&xsh[wv][16 * lane + 1024 * c + 4 * v]) = make_float4(xf[4 * v], xf[4 * v + 1], xf[4 * v + 2], xf[4 * v + 3]);
            }
        }
        lds_barrier();                                                           // (LDS only: the weight rows stay in flight)
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            q_f2 xp[NP][16];                                                         // (row 2q, row 2q + 1) of the lane's elements
#pragma unroll
            for (int q = 0; q < NP; ++q)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float4 a = *reinterpret_cast<const float4*>(&xsh[2 * q][16 * lane + 1024 * c + 4 * v]);
                    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (2 * q + 1 < NB) b = *reinterpret_cast<const float4*>(&xsh[2 * q + 1][16 * lane + 1024 * c + 4 * v]);
                    xp[q][4 * v] = (q_f2){a.x, b.x}; xp[q][4 * v + 1] = (q_f2){a.y, b.y};
                    xp[q][4 * v + 2] = (q_f2){a.z, b.z}; xp[q][4 * v + 3] = (q_f2){a.w, b.w};
                }
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                float wf[16];
                cvt16(wq[r][c], wf);
#pragma unroll
                for (int j = 0; j < 16; ++j)
#pragma unroll
                    for (int q = 0; q < NP; ++q) acc[r][q] = __builtin_elementwise_fma((q_f2){wf[j], wf[j]}, xp[q][j], acc[r][q]);
            }
            if constexpr (KC > 2) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (EK == 2 && KC > 2) ext_fetch();
    float sc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) sc[r] = scale[nn * RW + r];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float a0 = (b & 1) ? acc[0][b >> 1].y : acc[0][b >> 1].x;
        float v;
        [[maybe_unused]] bool ron = false;                       // (wave-uniform) the row has an adapter
        if constexpr (EK == 2) ron = ea[b] >= 0;
        if constexpr (SWIGLU) {
            // both row sums in one butterfly (gemv_reg_kernel): gate partials to lanes 0-31, up partials to lanes 32-63
            const float a1 = (b & 1) ? acc[1][b >> 1].y : acc[1][b >> 1].x;
            float gs, us;
            wave_sum2(a0, a1, gs, us);
            gs *= sc[0];
            us *= sc[1];
            if constexpr (EK == 2) {
                if (ron) {
                    // the extension's own butterfly, the same pairing: lane partials from zero, gate to lanes 0-31, up to 32-63
                    float ge, ue;
                    wave_sum2(ext_fma(0.f, eb[0][b], et[b]), ext_fma(0.f, eb[1][b], et[b]), ge, ue);
                    gs += ge;
                    us += ue;
                    gs += ebias[0][b];
                    us += ebias[1][b];
                }
            }
            const float g = bf2f(f2bf(gs)), u = bf2f(f2bf(us));
            v = silu(g) * u;
        } else {
            v = wave_sum(a0) * sc[0];
            if constexpr (EK == 2) {
                if (ron) {
                    v += wave_sum(ext_fma(0.f, eb[0][b], et[b]));
                    v += ebias[0][b];
                }
            }
        }
        if (lane == 0 && live) {
            if (R) v += bf2f(R[(size_t)b * ldy + n]);
            if constexpr (sizeof(OutT) == 2) y[(size_t)b * ldy + n] = f2bf(v);
            else y[(size_t)b * ldy + n] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- five to sixteen batch rows
// gemv_mfma_kernel<WeightFp8, ...> of gemv_mfma.h: the bf16 product's kernel with the weight fragments converted from e4m3 in
// registers and the finished row sum scaled by scale[n].  FP8-specific is only the layout that makes this possible: a lane's 16
// weights of a 64-k step are ONE 16-byte load, whose bytes 0-7 and 8-15 are the fragments of the step's two MFMAs - the k
// ownership of the bf16 weights' two loads, element for element.  So the product differs from the bf16 product on the dequantised
// weights by the scale's place only, and not at all where the scale is a power of two (scaling by it commutes with every
// rounding): FP8 mode and bf16 mode then decode the same bits.  The other layout - 128-k steps, 32 bytes per lane, a whole 128-byte
// line per row as the bf16 kernel fetches - was built first and measured 7-21 % faster per product than bf16; it sums in another
// order, and on weights both modes hold exactly the two modes' sampled codes then drift apart inside a frame ('FP8
// weights').

}  // namespace

extern "C" int csm_quantize_rows_fp8(const void* W, void* W8, void* scale, int N, int K, int ldw, int ldw8, hipStream_t stream) {
    CSM_REQUIRE(W && W8 && scale && N > 0 && K > 0, "csm_quantize_rows_fp8: bad arguments (N=%d K=%d)", N, K);
    CSM_REQUIRE((K & 7) == 0 && (ldw & 7) == 0 && (ldw8 & 7) == 0 && ldw >= K && ldw8 >= K,
                "csm_quantize_rows_fp8: K, ldw and ldw8 must be multiples of 8 and the leading dimensions >= K (K=%d ldw=%d ldw8=%d)",
                K, ldw, ldw8);
    CSM_REQUIRE(((uintptr_t)W & 15) == 0 && ((uintptr_t)W8 & 7) == 0, "csm_quantize_rows_fp8: W must be 16-byte and W8 8-byte aligned");
    hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, (const bf16_t*)W, (uint8_t*)W8, (float*)scale,
                       N, K, ldw, ldw8);
    CSM_CHECK_LAUNCH("csm_quantize_rows_fp8");
    return 0;
}

// ext: empty (csm_gemv_fp8w) or one GemvExtRows (csm_gemv_fp8w_kext_rows): the same checks and dispatch, the kernels' trailing pack
template <typename... Ext>
static int gemv_fp8_launch(const void* x, const void* W8, const void* scale, void* y, const void* residual, int B, int N, int K,
                           int ldw8, int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu,
                           const int* row_index, int row_offset, hipStream_t stream, Ext... ext) {
    constexpr bool EXT = ExtKind<Ext...>::v != 0;
    CSM_REQUIRE(x && W8 && scale && y && B >= 1 && B <= 16 && N > 0 && K > 0,
                "csm_gemv_fp8w: bad arguments (B=%d N=%d K=%d: needs 1 <= B <= 16)", B, N, K);
    CSM_REQUIRE((K & 15) == 0 && K <= 8192, "csm_gemv_fp8w: needs K %% 16 == 0 and K <= 8192 (K=%d): a 16-byte load carries 16 weights", K);
    CSM_REQUIRE((ldw8 & 15) == 0 && ldw8 >= K && ((uintptr_t)W8 & 15) == 0,
                "csm_gemv_fp8w: needs ldw8 %% 16 == 0, ldw8 >= K and a 16-byte aligned W8 (ldw8=%d K=%d)", ldw8, K);
    CSM_REQUIRE((ldx & 7) == 0 && ((uintptr_t)x & 15) == 0, "csm_gemv_fp8w: needs ldx %% 8 == 0 and a 16-byte aligned x (ldx=%d)", ldx);
    CSM_REQUIRE(!norm_scale || ((uintptr_t)norm_scale & 15) == 0, "csm_gemv_fp8w: norm_scale must be 16-byte aligned");
    CSM_REQUIRE(!swiglu || ((N & 1) == 0 && !out_f32), "csm_gemv_fp8w: the SwiGLU form needs an even N and bf16 output");
    const bool nt = K == 2048 || (K == 8192 && N == 2048);   // the 2048-wide stack: streamed once per frame, non-temporal
    if (B > 4)                                                // gemv_mfma.h
        return gemv_mfma_launch<WeightFp8>({(const uint8_t*)W8, (const float*)scale}, x, y, residual, B, N, K, ldw8, ldx, ldy, out_f32, norm_scale,
                                           eps, swiglu, row_index, row_offset, nt, stream, ext...);
#define ARGS(T) (const bf16_t*)x, (const uint8_t*)W8, (const float*)scale, (T*)y, (const bf16_t*)residual
    const int no = swiglu ? N / 2 : N;
    const int grid = (no + 3) / 4;
    const int kc = K <= 1024 ? 1 : (K <= 2048 ? 2 : 8);
    const size_t lds = B == 1 ? 0 : (size_t)B * kc * 1024 * sizeof(float);
#define LN(KC, NB, T, SW, NT_) do { auto kf = gemv_fp8_kernel<KC, NB, T, SW, NT_, Ext...>;                                              \
        if (lds > 65536) { static bool done_ = false; if (!done_) { (void)hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); done_ = true; } } \
        hipLaunchKernelGGL(kf, dim3(grid), dim3(256), lds, stream, ARGS(T), N, K, ldw8, ldx, ldy, (const bf16_t*)norm_scale, eps, row_index, row_offset, ext...); } while (0)
#define LNB(KC, T, SW, NT_) do { if (B == 1) LN(KC, 1, T, SW, NT_); else if (B == 2) LN(KC, 2, T, SW, NT_); else if (B == 3) LN(KC, 3, T, SW, NT_); else LN(KC, 4, T, SW, NT_); } while (0)
#define LNK(T, SW) do { if (kc == 1) LNB(1, T, SW, false); else if (kc == 2) { if (nt) LNB(2, T, SW, true); else LNB(2, T, SW, false); } \
                        else { if (nt) LNB(8, T, SW, true); else LNB(8, T, SW, false); } } while (0)
    if (swiglu) LNK(bf16_t, true); else if (out_f32) LNK(float, false); else LNK(bf16_t, false);
#undef LNK
#undef LNB
#undef LN
#undef ARGS
    if (EXT)
        g_last_gemv = {B == 1 ? "gemv_fp8_kernel<%d, 1, %s, %d, %d, ext2>" : B == 2 ? "gemv_fp8_kernel<%d, 2, %s, %d, %d, ext2>"
                       : B == 3 ? "gemv_fp8_kernel<%d, 3, %s, %d, %d, ext2>" : "gemv_fp8_kernel<%d, 4, %s, %d, %d, ext2>",
                       (out_f32 && !swiglu) ? "float" : "bf16", {kc, swiglu ? 1 : 0, (nt && kc != 1) ? 1 : 0, 0, 0, 0}};
    else
        g_last_gemv = {B == 1 ? "gemv_fp8_kernel<%d, 1, %s, %d, %d>" : B == 2 ? "gemv_fp8_kernel<%d, 2, %s, %d, %d>"
                       : B == 3 ? "gemv_fp8_kernel<%d, 3, %s, %d, %d>" : "gemv_fp8_kernel<%d, 4, %s, %d, %d>",
                       (out_f32 && !swiglu) ? "float" : "bf16", {kc, swiglu ? 1 : 0, (nt && kc != 1) ? 1 : 0, 0, 0, 0}};
    CSM_CHECK_LAUNCH("csm_gemv_fp8w");
    return 0;
}

extern "C" int csm_gemv_fp8w(const void* x, const void* W8, const void* scale, void* y, const void* residual, int B, int N, int K,
                             int ldw8, int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu,
                             const int* row_index, int row_offset, hipStream_t stream) {
    return gemv_fp8_launch(x, W8, scale, y, residual, B, N, K, ldw8, ldx, ldy, out_f32, norm_scale, eps, swiglu, row_index, row_offset, stream);
}

// csm_gemv_fp8w with one adapter per batch row (GemvExtRows, as csm_gemv_bf16_kext_rows takes it): B = 1..16.
extern "C" int csm_gemv_fp8w_kext_rows(const void* x, const void* W8, const void* scale, void* y, const void* residual, int B, int N,
                                       int K, int ldw8, int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu,
                                       const int* row_index, int row_offset, const void* ext_t, const void* const* ext_B,
                                       const void* const* bias, const int* row_adapter, int n_adapters, int kx, int ld_ext_t,
                                       int ld_ext_B, hipStream_t stream) {
    GemvExtRows e;
    if (const int rc = ext_rows_check("csm_gemv_fp8w_kext_rows", e, B, ext_t, ext_B, bias, row_adapter, n_adapters, kx, ld_ext_t, ld_ext_B)) return rc;
    return gemv_fp8_launch(x, W8, scale, y, residual, B, N, K, ldw8, ldx, ldy, out_f32, norm_scale, eps, swiglu, row_index, row_offset, stream, e);
}
