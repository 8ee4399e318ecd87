// The K-extension of the decode products, shared by the bf16 families (generate.hip) and the FP8 families (quant.hip): the
// argument packs, the per-row adapter lookup and the extension's arithmetic.  Everything here sits in the including file's
// anonymous namespace; it needs common.h (bf16_t, U4, unpack8, bf2f).
#pragma once
#include "common.h"

namespace {

// K-extension of a decode product (a LoRA group, training/lora.py): output row n also takes sum_j t[b][j] Bx[n][j] (+ bias[n])
// - the group's adapters as extra k-steps of the frozen projection, before the residual / SwiGLU / fp32-output epilogue, as
// csm_gemm_bf16_kext does in training.  The kernels below take it as a trailing argument PACK: the plain instantiations have an
// empty pack, so their signature and code are what they were.  Lane l owns the extension's 8-element chunk l (kx <= 512), loaded
// beside the weights; its products are added to the lane's partial sum AFTER the main k-loop (the main partial sums keep their
// order: Bx = 0 leaves every bit of the plain product) by explicit fused multiply-adds in ascending j - the same operations in
// every kernel, so a B-row launch stays bit-equal per row to the one-row launch.
struct GemvExt {
    const bf16_t* t;      // [B][ldt]  s x^ At, bf16 (csm_lora_project_bf16)
    const bf16_t* Bx;     // [N][ldb]  rows in the fused projection's order (w13: gate / up interleaved)
    const bf16_t* bias;   // [N] or NULL
    int kx, ldt, ldb;
};
__device__ __forceinline__ const GemvExt& ext_arg(const GemvExt& e) { return e; }
// The per-row ("gathered") form (csm_gemv_bf16_kext_rows: a bank of adapters, one per batch row): row b takes its extension from
// adapter a = row_adapter[b] - Bx[a], bias[a] (the table itself or an entry may be NULL) - with the same operations in the same
// order as GemvExt, so row b is bit-identical to a one-row GemvExt launch with adapter a.  a = -1 (or out of range): no extension
// at all, the plain product's bits.  t is [B][ldt] as for GemvExt (csm_lora_project_rows_bf16 leaves each row's own adapter's t).
struct GemvExtRows {
    const bf16_t* t;                  // [B][ldt]
    const bf16_t* const* Bx;          // [nad] -> [N][ldb]
    const bf16_t* const* bias;        // [nad] -> [N] or NULL; NULL: no adapter has a bias
    const int* row_adapter;           // [B], -1 = none
    int nad, kx, ldt, ldb;
};
__device__ __forceinline__ const GemvExtRows& ext_rows_arg(const GemvExtRows& e) { return e; }
// 0: the plain products (empty pack), 1: GemvExt, 2: GemvExtRows
template <typename... E> struct ExtKind { static constexpr int v = 0; };
template <> struct ExtKind<GemvExt> { static constexpr int v = 1; };
template <> struct ExtKind<GemvExtRows> { static constexpr int v = 2; };
__device__ __forceinline__ int ext_row_adapter(const GemvExtRows& e, int b) {      // (wave-uniform) the row's adapter or -1
    const int a = e.row_adapter[b];
    return a < e.nad ? a : -1;
}
__device__ __forceinline__ float ext_row_bias(const GemvExtRows& e, int a, int n) {
    const bf16_t* bb = e.bias ? e.bias[a] : nullptr;
    return bb ? bf2f(bb[n]) : 0.f;
}
__device__ __forceinline__ U4 ext_load(const bf16_t* row, int lane, int kx) {
    U4 z = {0u, 0u, 0u, 0u};
    return lane < (kx >> 3) ? *reinterpret_cast<const U4*>(row + lane * 8) : z;
}
__device__ __forceinline__ float ext_fma(float acc, const U4& b, const U4& t) {
    float bf[8], tf[8];
    unpack8(b, bf);
    unpack8(t, tf);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(bf[j], tf[j], acc);
    return acc;
}
// the whole extension of one output on one thread (the MFMA kernels' epilogue): one fmaf per j onto v, in ascending j
__device__ __forceinline__ float ext_dot(float v, const bf16_t* __restrict__ bx, const bf16_t* __restrict__ t, int kx) {
    for (int j = 0; j < kx; j += 8)
        v = ext_fma(v, *reinterpret_cast<const U4*>(bx + j), *reinterpret_cast<const U4*>(t + j));
    return v;
}

// host: the checks of a per-row extension's arguments, shared by the *_kext_rows entry points (`entry`: the caller's name, for the
// message); fills e
static inline int ext_rows_check(const char* entry, GemvExtRows& e, int B, const void* ext_t, const void* const* ext_B,
                                 const void* const* bias, const int* row_adapter, int n_adapters, int kx, int ld_ext_t, int ld_ext_B) {
    CSM_REQUIRE(B >= 1 && B <= 16, "%s: B=%d: the per-row K-extension takes 1 to 16 batch rows", entry, B);
    CSM_REQUIRE(ext_t && ext_B && row_adapter && n_adapters >= 1 && kx > 0 && kx <= 512 && (kx & 7) == 0 && ld_ext_t >= kx &&
                ld_ext_B >= kx && (ld_ext_t & 7) == 0 && (ld_ext_B & 7) == 0 && ((uintptr_t)ext_t & 15) == 0,
                "%s: bad extension (adapters=%d kx=%d ld_t=%d ld_B=%d: needs kx <= 512, multiples of 8, 16-byte aligned rows)",
                entry, n_adapters, kx, ld_ext_t, ld_ext_B);
    e.t = (const bf16_t*)ext_t; e.Bx = (const bf16_t* const*)ext_B; e.bias = (const bf16_t* const*)bias;
    e.row_adapter = row_adapter; e.nad = n_adapters; e.kx = kx; e.ldt = ld_ext_t; e.ldb = ld_ext_B;
    return 0;
}

}  // namespace
