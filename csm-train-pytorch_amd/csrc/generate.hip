// Generation-side kernels for gfx950: top-k / temperature sampler with injected Exp(1) noise, and the Mimi
// split residual vector quantiser (nearest-codeword encode, codebook-sum decode).
#include "common.h"
#include "gemv_ext.h"
#include "gemv_mfma.h"
#include <math.h>

namespace {

// Probe builds only (-DCSM_DECODE_STAMPS, tools/probes/decode_stamps.sh): the first and the last workgroup of a stamped kernel
// record the 100 MHz wall clock at a few points; the product build compiles none of this.
#ifdef CSM_DECODE_STAMPS
__device__ unsigned long long g_decode_stamps[8192];
__device__ unsigned int g_decode_nstamp;
#define STAMP_DECL unsigned long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define STAMP(i) do { __builtin_amdgcn_sched_barrier(0); st_[i] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_FLUSH(id) do { if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) {                          \
        const unsigned int s0 = atomicAdd(&g_decode_nstamp, 10u);                                                                   \
        if (s0 + 10 <= 8192) { g_decode_stamps[s0] = (id); g_decode_stamps[s0 + 1] = blockIdx.x;                                    \
            for (int q_ = 0; q_ < 8; ++q_) g_decode_stamps[s0 + 2 + q_] = st_[q_]; } } } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH(id)
#endif

struct ValIdx { float v; int i; };

__device__ __forceinline__ ValIdx vi_max(ValIdx a, ValIdx b) {  // larger value wins, then the lower index
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ ValIdx vi_min(ValIdx a, ValIdx b) {  // smaller value wins, then the lower index
    return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

template <bool MAX>
__device__ __forceinline__ ValIdx block_arg(ValIdx x, ValIdx* red) {
#define CSM_ARG_STEP(o) { ValIdx y; y.v = lane_xor<o>(x.v); y.i = lane_xor<o>(x.i); x = MAX ? vi_max(x, y) : vi_min(x, y); }
    CSM_ARG_STEP(32) CSM_ARG_STEP(16) CSM_ARG_STEP(8) CSM_ARG_STEP(4) CSM_ARG_STEP(2) CSM_ARG_STEP(1)
#undef CSM_ARG_STEP
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = x;
    __syncthreads();
    ValIdx r = red[0];
    for (int k = 1; k < nw; ++k) r = MAX ? vi_max(r, red[k]) : vi_min(r, red[k]);
    return r;
}

// reference src/csm/models/model.py:79-96: logits/T, keep values >= k-th largest, log_softmax -> softmax,
// argmax(p / q) with q ~ Exp(1) supplied by the caller.  One 256-thread block per row, V <= 256 * NPT.
// A generated frame draws 32 codes one after the other, so this kernel's latency is paid 32 times per 80 ms of audio; it runs as
// ONE workgroup on a cold CU, and what it costs is latency, not work (tools/probes/decode_stamps.py, round 4: of 15 us, 4-5
// were the Exp(1) row arriving from HBM right before the last step, 5-6 the 9-16 rounds of the bisection that found the k-th
// largest value, 2-3 the logits' own arrival).  So:
//  * the Exp(1) row is requested first of all and consumed last;
//  * the k-th largest value comes from an 8-bit radix select on an order-preserving integer image of the floats: per pass the
//    keys that still match the prefix are counted into a 256-bin LDS histogram (ds_add_u32; four histograms, zeroed once, so a
//    pass needs ONE barrier), every wave then scans the bins from the top (4 bins per lane, a DPP row scan + three row totals, no
//    LDS crossbar) and reads the digit, the count above it and the count inside it off the lane that crosses k.  At most four
//    passes; a pass whose digit leaves exactly the wanted number of keys at or above it ends the search (the kept set is decided:
//    typical logits separate their 50th and 51st value in the second pass).  Rounds 2-3 used a bisection with ballots: 2 bits per
//    round, 9-16 rounds of ~0.35 us.
// The kept set is `key >= threshold` on the integer image - the set `value >= k-th largest` keeps (ties included).
constexpr int SMP_PER_THREAD = 16;
__device__ __forceinline__ int dpp_row_shr_add(int v, int ctrl_n) {   // v + (v shifted right by n lanes inside its row of 16, zero fill)
    switch (ctrl_n) {
        case 1: return v + __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
        case 2: return v + __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
        case 4: return v + __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
        default: return v + __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    }
}
// Where a row's two parameters come from (the kernel's last template parameter).  SampleScalars: the launch scalars of
// csm_sample_topk, one pair for every row, validated by the entry point - the kernel argument layout (int, float) and the code
// are those of the kernel before there were two forms.  SampleRows (csm_sample_topk_rows): row r samples with topk[r] /
// temperature[r], read from device memory - so a captured frame serves every mix of parameters (csm/serving.py,
// row_sampling).  The two are loaded once per workgroup (two scalar loads of block-uniform addresses, issued among the Exp(1)
// row's and the logits' loads and before the first wait on any of them, so all are in flight together; the division is their
// first use).  The host cannot see them, so they are made safe here: top-k into [1, V]; a temperature that is not a finite
// positive number (zero, negative, NaN, inf) counts as 1.  The one-wave / block-wide choice stays block-uniform: a workgroup
// is one row.
struct SampleScalars {
    static constexpr bool FILTERS = false, PENALTY = false, TYPICAL = false;
    int topk;
    float temperature;
    __device__ __forceinline__ int k(int, int) const { return topk; }
    __device__ __forceinline__ float t(int) const { return temperature; }
};
struct SampleRows {
    static constexpr bool FILTERS = false, PENALTY = false, TYPICAL = false;
    const int* topk;
    const float* temperature;
    __device__ __forceinline__ int k(int row, int V) const { const int v = topk[row]; return v < 1 ? 1 : (v > V ? V : v); }
    __device__ __forceinline__ float t(int row) const { const float v = temperature[row]; return (v > 0.f && v < INFINITY) ? v : 1.f; }
};
// SampleFiltered (csm_sample_filtered_rows): SampleRows plus a nucleus (top-p) and a min-p threshold per row, two more
// block-uniform loads issued with the other two.  With v = x / temperature, e_i = exp(v_i - max v) and K today's kept set:
//   M = { i in K : e_i >= min_p };  N = { i in M : sum over j in M with v_j > v_i of e_j  <  top_p * sum over M of e_j };
// the finish (log_softmax -> softmax -> argmax p / q) then runs over N with today's expressions.  Every rule is a threshold on
// the value - equal values stay or go together and no index enters - so N is never empty (nothing lies above the largest).
// A top_p outside (0, 1] counts as 1, a min_p outside [0, 1] as 0 (NaN is outside both).  A row with (1, 0) skips all of it
// (block-uniform) and is the SampleRows kernel.  Mass is summed as 64-bit fixed point, e_i * 2^40 truncated: integer sums do
// not depend on their order, so neither the butterfly nor the LDS atomics below can change a kept set from run to run.
//  * at most 64 kept values (the common case after top-k): wave 0 has them compacted, one per lane; every lane walks the
//    others' (value, mass) pairs with readlane and adds up the mass strictly above its own value.
//  * more: a second 8-bit radix select over the same integer keys, with the mass instead of a count added into 64-bit LDS
//    histograms (ds_add_u64); the wanted mass tau = ceil(top_p * S) plays the part of k.  The digit's bin is the first from the
//    top whose inclusive mass reaches tau: the bins above it are kept whole, the ones below dropped whole, and tau minus the mass
//    above (exact in integers) is wanted inside it.  Four passes give the last kept key; rows that min-p drops get key 0, which
//    no threshold keeps.  The set is then counted again and takes whichever finish fits it.
// Error: |kernel's sum P_j - exact| <= 2 (V 2^-40 + (2 + dbar) 2^-24), dbar the P-weighted mean of
// max v - v_j; |kernel's e_i / exact - 1| <= (2 + max v - v_i) 2^-24.
struct SampleFiltered : SampleRows {
    static constexpr bool FILTERS = true, PENALTY = false, TYPICAL = false;
    const float* top_p;
    const float* min_p;
    __device__ __forceinline__ float p(int row) const { const float v = top_p[row]; return (v > 0.f && v <= 1.f) ? v : 1.f; }
    __device__ __forceinline__ float m(int row) const { const float v = min_p[row]; return (v >= 0.f && v <= 1.f) ? v : 0.f; }
};
// SampleProcessed (csm_sample_processed_rows): SampleFiltered plus a windowed repetition penalty and the row's memory of what it
// drew.  A row keeps, per codebook, a ring of SMP_HIST codes: slot f % SMP_HIST holds the code of frame f of its utterance.  With
// f = frame[row] and n = min(window[row], f, SMP_HIST), the distinct ids of ring[(f - 1 - j) % SMP_HIST], j < n, that lie in
// [0, V) get x = x > 0 ? x / r : x * r - ONE correctly rounded fp32 operation on the raw logit, before the division by the
// temperature; an id seen twice is penalised once, ids outside [0, V) are ignored (so a ring nobody initialised is harmless).
// A penalty that is not a finite positive number counts as 1, the window is clamped to [0, SMP_HIST].  r = 1 or n = 0 skips all
// of it (block-uniform) and is the SampleFiltered kernel.  How: wave 0 loads the ring, one slot per lane, and builds a V-bit
// membership bitmap in LDS (it zeroes the 72 / 128 words, then every lane whose slot the window reaches ORs its bit in: one ds_or;
// a readlane walk over the entries cost 80 ns per entry, 5 us at n = 64) while the other waves zero the histograms; one more
// barrier publishes it, and every thread tests its own bits before it forms x / temperature.  The
// ring, the penalty, the window, the frame and the live flag are loads of block-uniform or per-lane addresses issued with the
// logits' and the Exp(1) row's, so all are in flight together.  A live row then stores its winner to ring[f % SMP_HIST] (after
// every read of the ring: the reads sit before the first barrier, the store after the last; with n = SMP_HIST it overwrites the
// oldest entry read) and, with `advance`, f + 1 to frame[row] - plain vector stores by the thread that writes `out`.  Only this
// row's block touches the row's ring and counter.
constexpr int SMP_HIST = 64;
struct SampleProcessed : SampleFiltered {
    static constexpr bool FILTERS = true, PENALTY = true, TYPICAL = false;
    const float* penalty;
    const int* window;
    int* hist;
    int ldh;
    int* frame;
    const int* live;
    int advance;
    __device__ __forceinline__ float r(int row) const { const float v = penalty[row]; return (v > 0.f && v < INFINITY) ? v : 1.f; }
    __device__ __forceinline__ int w(int row) const { const int v = window[row]; return v < 0 ? 0 : (v > SMP_HIST ? SMP_HIST : v); }
    __device__ __forceinline__ void wrote(int row, int f, int winner) const {   // (one thread, after the draw)
        if (live[row]) {
            hist[(size_t)row * ldh + (f & (SMP_HIST - 1))] = winner;
            if (advance) frame[row] = f + 1;
        }
    }
};
// SampleTypical (csm_sample_typical_rows): SampleProcessed plus locally typical sampling (Meister et al. 2022) per row, one more
// block-uniform load issued with the others.  It comes last, on the set N the nucleus leaves.  With P_i = e_i / sum_N e_j,
// h_i = -ln P_i = d_i + ln sum_N e_j (d_i = max v - v_i) and H = sum_N P_i h_i, a token's distance from typical is
//   delta_i = |h_i - H| = |d_i - D|,  D = sum_N P_i d_i    (ln sum_N e_j is in h_i and in H alike: it is never formed),
//   T = { i in N : sum over j in N with delta_j < delta_i of P_j  <  typical_p };
// the token that crosses typical_p is kept, equal values have equal delta and stay or go together, and nothing lies below the
// smallest delta, so T is never empty - but it need not hold the largest value: the finish takes its max over T.  A typical_p
// outside (0, 1] (NaN included) counts as 1, and 1 skips all of it (block-uniform): the SampleProcessed kernel.
// D is ONE number per row: e_i d_i is summed in the mass's 2^-40 fixed point beside e_i (integer sums: any order gives the same
// bits), D = (float)((double)W / (double)S), and delta_i = fabsf(d_i - D) sees the token's value and D only.
//  * at most 64 values in N: in the one-wave finish, after the nucleus - two wave sums, delta per lane, then the nucleus's
//    readlane walk with `delta_j < delta_i` for `v_j > v_i`.
//  * more: smp_mass_select a second time, on the key ~bits(delta) (delta >= 0: its bit pattern is ordered, and complemented the
//    most typical comes first; never 0, which stays "not in N").  The 8 KB of mass histograms are zeroed again after the count
//    that follows the nucleus.  Seven barriers: one for the sums and the zeroes, four passes, two for the count of T.
// Error: |kernel's delta_i - exact| <= 2 a + (2 max_N d + D) 2^-24 with
// a = (6 D + D2 + D^2) 2^-24 + (1 + D) V 2^-40, D2 = sum_N P_i d_i^2; the mass sums are the nucleus's.
struct SampleTypical : SampleProcessed {
    static constexpr bool FILTERS = true, PENALTY = true, TYPICAL = true;
    const float* typical_p;
    __device__ __forceinline__ float y(int row) const { const float v = typical_p[row]; return (v > 0.f && v <= 1.f) ? v : 1.f; }
};
constexpr float SMP_MASS_ONE = 1099511627776.f;                          // 2^40: the fixed-point image of e = 1
__device__ __forceinline__ unsigned long long smp_mass(float e) { return (unsigned long long)(e * SMP_MASS_ONE); }   // (exact product, truncated)
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long smp_tau(unsigned long long S, float top_p) {   // smallest integer >= top_p * S (S < 2^53: exact)
    return (unsigned long long)ceil((double)S * (double)top_p);
}
// D = W / S: both below 2^53, so exact as doubles; the quotient is rounded to fp32 once more
__device__ __forceinline__ float smp_mean(unsigned long long W, unsigned long long S) {
    return (float)((double)W / (double)S);
}
// The block-wide mass select of the nucleus and of typical sampling: the last key, from the top, that is kept when `trem` of the
// mass of the keys >= lo is wanted - the largest key whose mass at or above it reaches trem.  Token j's mass is
// smp_mass(expf(val[j] - gtop)); mhist is zeroed and published by the caller.  Four 8-bit passes, one barrier each; the digit's
// bin is the first from the top whose inclusive mass reaches trem, and trem minus the mass above it is wanted inside it.
template <int NPT>
__device__ __forceinline__ uint32_t smp_mass_select(const uint32_t (&key)[NPT], const float (&val)[NPT], float gtop, uint32_t lo,
                                                    unsigned long long trem, unsigned long long (*mhist)[256], int V, int lane) {
    uint32_t mprefix = 0u;
#pragma unroll 1
    for (int ps = 0; ps < 4; ++ps) {
        const int shift = 24 - 8 * ps;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int c = threadIdx.x + 256 * j;
            const bool in = c < V && key[j] >= lo && (ps == 0 || (key[j] >> (shift + 8)) == (mprefix >> (shift + 8)));
            if (in) atomicAdd(&mhist[ps][(key[j] >> shift) & 255u], smp_mass(expf(val[j] - gtop)));
        }
        __syncthreads();
        // lane l owns bins 252 - 4l .. 255 - 4l, as in the count select; the scan runs from the top bin down
        const ulonglong2 hlo = *reinterpret_cast<const ulonglong2*>(&mhist[ps][252 - 4 * lane]);
        const ulonglong2 hhi = *reinterpret_cast<const ulonglong2*>(&mhist[ps][254 - 4 * lane]);
        const unsigned long long b3 = hhi.y, b2 = hhi.x, b1 = hlo.y, b0 = hlo.x;
        const unsigned long long mn = b3 + b2 + b1 + b0;
        unsigned long long pr = mn;             // -> mass in my bins and every bin above them
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long y = __shfl_up(pr, o, 64);
            if (lane >= o) pr += y;
        }
        unsigned long long above = pr - mn;
        int digit;
        if (above + b3 >= trem) digit = 255 - 4 * lane;
        else {
            above += b3;
            if (above + b2 >= trem) digit = 254 - 4 * lane;
            else {
                above += b2;
                if (above + b1 >= trem) digit = 253 - 4 * lane;
                else { above += b1; digit = 252 - 4 * lane; }
            }
        }
        const unsigned long long cross = __ballot(pr >= trem);
        const int L = cross ? __ffsll((long long)cross) - 1 : 63;          // (never empty: the matching mass is >= trem)
        digit = __builtin_amdgcn_readlane(digit, L);
        above = readlane_u64(above, L);
        mprefix |= (uint32_t)digit << shift;
        trem -= above;
    }
    return mprefix;
}
// The kept keys (>= prefix) of this thread, and with them the inclusive count over the wave's lanes up to this one.
template <int NPT>
__device__ __forceinline__ int smp_count_kept(const uint32_t (&key)[NPT], uint32_t prefix, int V, int lane, int& mine) {
    mine = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) mine += (threadIdx.x + 256 * j < V && key[j] >= prefix) ? 1 : 0;
    int pre = mine;
    pre = dpp_row_shr_add(pre, 1); pre = dpp_row_shr_add(pre, 2); pre = dpp_row_shr_add(pre, 4); pre = dpp_row_shr_add(pre, 8);
    const int t0 = __builtin_amdgcn_readlane(pre, 15), t1 = __builtin_amdgcn_readlane(pre, 31), t2 = __builtin_amdgcn_readlane(pre, 47);
    pre += (lane >= 16 ? t0 : 0) + (lane >= 32 ? t1 : 0) + (lane >= 48 ? t2 : 0);
    return pre;
}
template <int NPT, class Params>
__global__ __launch_bounds__(256) void sample_topk_kernel(const float* __restrict__ logits, const float* __restrict__ q,
                                                          int* __restrict__ out, int V, int ldl, const Params prm) {
    __shared__ ValIdx red[4];
    __shared__ float fred[16];
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][256];
    const int row = blockIdx.x;
    const int topk = prm.k(row, V);
    const float temperature = prm.t(row);
    float top_p = 1.f, min_p = 0.f;
    if constexpr (Params::FILTERS) { top_p = prm.p(row); min_p = prm.m(row); }
    float typical_p = 1.f;
    if constexpr (Params::TYPICAL) typical_p = prm.y(row);
    const float* x = logits + (size_t)row * ldl;
    const float* qq = q + (size_t)row * V;
    const int lane = threadIdx.x & 63;
    STAMP_DECL;
    STAMP(0);
    float rep = 1.f;
    int pframe = 0, pn = 0, recent = -1;
    if constexpr (Params::PENALTY) {
        // (wave 0's lane l takes slot l of the ring, whatever the frame is: the load depends on no other load)
        if (threadIdx.x < SMP_HIST) recent = prm.hist[(size_t)row * prm.ldh + threadIdx.x];
        rep = prm.r(row);
        pframe = prm.frame[row];
        const int w = prm.w(row);
        pn = __builtin_amdgcn_readfirstlane(pframe < w ? (pframe < 0 ? 0 : pframe) : w);        // min(window, frame, SMP_HIST)
    }
    const bool pen_on = Params::PENALTY && rep != 1.f && pn > 0;         // (block-uniform)
    float qv[NPT], val[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = threadIdx.x + 256 * j;
        val[j] = c < V ? x[c] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = threadIdx.x + 256 * j;
        qv[j] = c < V ? qq[c] : 1.f;
    }
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) hist[ps][threadIdx.x] = 0u;
    if constexpr (Params::PENALTY) {
        constexpr int PEN_WORDS = 256 * NPT / 32;           // the membership bitmap: one bit per id (72 or 128 words)
        __shared__ uint32_t pbits[PEN_WORDS];
        if (pen_on) {
            if (threadIdx.x < 64) {                         // wave 0: lane l zeroes words l, l + 64, then sets its slot's bit
                pbits[lane] = 0u;
                if (lane + 64 < PEN_WORDS) pbits[lane + 64] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // (one wave: its LDS operations complete in order)
                __builtin_amdgcn_wave_barrier();
                // V <= 256 * NPT: the word lies inside pbits.  An OR does not depend on the order of the lanes: the same bitmap
                // every run, and an id that is in the window twice sets one bit
                const int age = (pframe - 1 - lane) & (SMP_HIST - 1);      // slot `lane` holds the code of frame f - 1 - age
                if (age < pn && (unsigned)recent < (unsigned)V) atomicOr(&pbits[recent >> 5], 1u << (recent & 31));
            }
            __syncthreads();                                // the bitmap (block-uniform branch)
#pragma unroll
            for (int j = 0; j < NPT; ++j) {                 // thread's id c = threadIdx.x + 256 j: word 8 j + threadIdx.x / 32
                const bool hit = (pbits[8 * j + (threadIdx.x >> 5)] >> (threadIdx.x & 31)) & 1u;
                if (hit) val[j] = val[j] > 0.f ? val[j] / rep : val[j] * rep;
            }
        }
    }
    uint32_t key[NPT];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = threadIdx.x + 256 * j;
        val[j] = c < V ? val[j] / temperature : -INFINITY;
        const uint32_t u = __float_as_uint(val[j]);
        key[j] = c >= V ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
        tmax = fmaxf(tmax, val[j]);
    }
    STAMP(1);
    __syncthreads();                                        // the zeroed histograms
    STAMP(2);
    uint32_t prefix = 0u;
    int krem = topk;                                        // keys still wanted among those that match the prefix
#pragma unroll 1
    for (int ps = 0; ps < 4; ++ps) {
        const int shift = 24 - 8 * ps;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int c = threadIdx.x + 256 * j;
            const bool in = c < V && (ps == 0 || (key[j] >> (shift + 8)) == (prefix >> (shift + 8)));
            if (in) atomicAdd(&hist[ps][(key[j] >> shift) & 255u], 1u);
        }
        __syncthreads();
        // lane l owns bins 252 - 4l .. 255 - 4l; the scan runs from the top bin down (every wave does it: no second barrier)
        const uint4 hv = *reinterpret_cast<const uint4*>(&hist[ps][252 - 4 * lane]);
        const int b3 = (int)hv.w, b2 = (int)hv.z, b1 = (int)hv.y, b0 = (int)hv.x;      // bins 255-4l, 254-4l, 253-4l, 252-4l
        const int mine = b3 + b2 + b1 + b0;
        int pre = mine;
        pre = dpp_row_shr_add(pre, 1); pre = dpp_row_shr_add(pre, 2); pre = dpp_row_shr_add(pre, 4); pre = dpp_row_shr_add(pre, 8);
        const int t0 = __builtin_amdgcn_readlane(pre, 15), t1 = __builtin_amdgcn_readlane(pre, 31), t2 = __builtin_amdgcn_readlane(pre, 47);
        pre += (lane >= 16 ? t0 : 0) + (lane >= 32 ? t1 : 0) + (lane >= 48 ? t2 : 0);     // keys in my bins and every bin above them
        int above = pre - mine, digit, inside;
        if (above + b3 >= krem) { digit = 255 - 4 * lane; inside = b3; }
        else {
            above += b3;
            if (above + b2 >= krem) { digit = 254 - 4 * lane; inside = b2; }
            else {
                above += b2;
                if (above + b1 >= krem) { digit = 253 - 4 * lane; inside = b1; }
                else { above += b1; digit = 252 - 4 * lane; inside = b0; }
            }
        }
        const unsigned long long cross = __ballot(pre >= krem);
        const int L = cross ? __ffsll((long long)cross) - 1 : 63;                       // (never empty: the matching keys number >= krem)
        digit = __builtin_amdgcn_readlane(digit, L);
        above = __builtin_amdgcn_readlane(above, L);
        inside = __builtin_amdgcn_readlane(inside, L);
        prefix |= (uint32_t)digit << shift;
        const bool exact = above + inside == krem;          // exactly k keys at or above this prefix: the kept set is decided
        krem -= above;
        if (exact) break;                                   // (block-uniform: every wave read the same histogram)
    }
    STAMP(3);
    // ---- the kept values (k of them, more only with ties at the threshold) are compacted - in index order of (thread, slot), by a
    //      block-wide prefix sum of the per-thread counts: deterministic - and ONE wave evaluates log_softmax -> softmax -> p / q ->
    //      argmax on them: two wave butterflies instead of seven block-wide reductions with their fourteen barriers, and 1 exp per
    //      kept value instead of 9 per thread.  Tokens outside the kept set have p = 0 and can never win the race (the largest
    //      kept p is >= 1 / count).  More than 64 kept values (ties, or topk > 64): the block-wide form below.
    __shared__ float cval[64], cq[64];
    __shared__ int cidx[64];
    __shared__ int wtot[4];
    int mine;
    int pre = smp_count_kept<NPT>(key, prefix, V, lane, mine);
    if (lane == 63) wtot[threadIdx.x >> 6] = pre;
    __syncthreads();
    const int w_ = threadIdx.x >> 6;
    int before = (w_ > 0 ? wtot[0] : 0) + (w_ > 1 ? wtot[1] : 0) + (w_ > 2 ? wtot[2] : 0);
    int total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    bool wave_filters = false;                              // steps 2 and 3 still to be done, by the one-wave finish
    bool typical = false;                                   // the typical step still to be done (block-uniform)
    bool typical_done = false;                              // ... or done: the finish takes its max over T
    if constexpr (Params::TYPICAL) typical = typical_p < 1.f;
    if constexpr (Params::FILTERS) {
        wave_filters = top_p < 1.f || min_p > 0.f;          // (block-uniform; false: the SampleRows kernel from here on)
        if ((wave_filters || typical) && total > 64) {
            // ---- more than 64 kept values: min-p and the nucleus block-wide, on the keys in registers
            __shared__ __attribute__((aligned(16))) unsigned long long mhist[4][256];
            __shared__ unsigned long long sred[4];
            wave_filters = false;
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) mhist[ps][threadIdx.x] = 0ull;
            const float gtop = block_max(tmax, fred);
            if (prefix == 0u) prefix = 1u;                  // (no value has key 0: the same set, and key 0 now means dropped)
            unsigned long long sm = 0ull;
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int c = threadIdx.x + 256 * j;
                if (c < V && key[j] >= prefix) {
                    const float e = expf(val[j] - gtop);
                    if (e >= min_p) sm += smp_mass(e);
                    else key[j] = 0u;                       // dropped by min-p: below every threshold (prefix >= 1)
                }
            }
            if (top_p < 1.f) {                              // (block-uniform)
                sm = wave_sum_u64(sm);
                if (lane == 0) sred[w_] = sm;
                __syncthreads();                            // the wave sums, and the zeroed histograms
                const unsigned long long trem = smp_tau(sred[0] + sred[1] + sred[2] + sred[3], top_p);   // mass still wanted
                // the last kept key (>= the top-k threshold: its bin held mass)
                prefix = smp_mass_select<NPT>(key, val, gtop, prefix, trem, mhist, V, lane);
            }
            // the kept set changed: count it again for the compaction
            pre = smp_count_kept<NPT>(key, prefix, V, lane, mine);
            __syncthreads();                                // every wave has read the first count
            if (lane == 63) wtot[w_] = pre;
            __syncthreads();
            before = (w_ > 0 ? wtot[0] : 0) + (w_ > 1 ? wtot[1] : 0) + (w_ > 2 ? wtot[2] : 0);
            total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
            if constexpr (Params::TYPICAL) {
                if (typical && total > 64) {
                    // ---- more than 64 values in N: typical block-wide.  Every wave is past the barriers of the count, so
                    //      nobody still reads the nucleus's histograms or sums
                    __shared__ unsigned long long tred[2][4];
                    typical = false;
                    typical_done = true;
#pragma unroll
                    for (int ps = 0; ps < 4; ++ps) mhist[ps][threadIdx.x] = 0ull;
                    unsigned long long ts = 0ull, tw = 0ull;            // sum e_i and sum e_i d_i over N, in 2^-40
#pragma unroll
                    for (int j = 0; j < NPT; ++j) {
                        const int c = threadIdx.x + 256 * j;
                        if (c < V && key[j] >= prefix) {
                            const float e = expf(val[j] - gtop);
                            ts += smp_mass(e);
                            if (e > 0.f) tw += smp_mass(e * (gtop - val[j]));
                        }
                    }
                    ts = wave_sum_u64(ts);
                    tw = wave_sum_u64(tw);
                    if (lane == 0) { tred[0][w_] = ts; tred[1][w_] = tw; }
                    __syncthreads();                        // the wave sums, and the zeroed histograms
                    const unsigned long long S = tred[0][0] + tred[0][1] + tred[0][2] + tred[0][3];
                    const float D = smp_mean(tred[1][0] + tred[1][1] + tred[1][2] + tred[1][3], S);
#pragma unroll
                    for (int j = 0; j < NPT; ++j) {         // the keys become ~bits(delta); 0: not in N
                        const int c = threadIdx.x + 256 * j;
                        key[j] = (c < V && key[j] >= prefix) ? ~__float_as_uint(fabsf((gtop - val[j]) - D)) : 0u;
                    }
                    prefix = smp_mass_select<NPT>(key, val, gtop, 1u, smp_tau(S, typical_p), mhist, V, lane);
                    pre = smp_count_kept<NPT>(key, prefix, V, lane, mine);
                    __syncthreads();                        // every wave has read the second count
                    if (lane == 63) wtot[w_] = pre;
                    __syncthreads();
                    before = (w_ > 0 ? wtot[0] : 0) + (w_ > 1 ? wtot[1] : 0) + (w_ > 2 ? wtot[2] : 0);
                    total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
                }
            }
        }
    }
    if (total <= 64) {                                      // (block-uniform)
        int at = before + pre - mine;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int c = threadIdx.x + 256 * j;
            if (c < V && key[j] >= prefix) { cval[at] = val[j]; cq[at] = qv[j]; cidx[at] = c; ++at; }
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            bool on = lane < total;
            float v = on ? cval[lane] : -INFINITY;
            float top = wave_max(v);
            if constexpr (Params::FILTERS) {
                if (wave_filters) {                         // steps 2 and 3 on the compacted values, one per lane
                    const float e = on ? expf(v - top) : 0.f;
                    on = on && e >= min_p;
                    const unsigned long long ms = on ? smp_mass(e) : 0ull;
                    if (top_p < 1.f) {
                        const unsigned long long tau = smp_tau(wave_sum_u64(ms), top_p);
                        unsigned long long above = 0ull;    // mass of the values strictly larger than mine
#pragma unroll 1
                        for (int j = 0; j < total; ++j) {
                            const float vj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), j));
                            const unsigned long long mj = readlane_u64(ms, j);
                            above += vj > v ? mj : 0ull;
                        }
                        on = on && above < tau;
                    }
                    v = on ? v : -INFINITY;
                }
            }
            if constexpr (Params::TYPICAL) {
                if (typical) {                              // the typical step on N, one value per lane
                    const float d = top - v;
                    const float e = on ? expf(v - top) : 0.f;
                    const unsigned long long ms = smp_mass(e);
                    const unsigned long long S = wave_sum_u64(ms);
                    const float D = smp_mean(wave_sum_u64(e > 0.f ? smp_mass(e * d) : 0ull), S);
                    const float delta = on ? fabsf(d - D) : INFINITY;
                    const unsigned long long tau = smp_tau(S, typical_p);
                    unsigned long long below = 0ull;        // mass of the values strictly more typical than mine
#pragma unroll 1
                    for (int j = 0; j < total; ++j) {
                        const float dj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(delta), j));
                        const unsigned long long mj = readlane_u64(ms, j);
                        below += dj < delta ? mj : 0ull;
                    }
                    on = on && below < tau;
                    v = on ? v : -INFINITY;
                    top = wave_max(v);                      // (T need not hold the largest value)
                }
            }
            const float e1 = on ? expf(v - top) : 0.f;
            const float logsum = logf(wave_sum(e1));
            const float ymax = (top - top) - logsum;
            const float e2 = on ? expf(((v - top) - logsum) - ymax) : 0.f;
            const float s2 = wave_sum(e2);
            ValIdx best = {-INFINITY, 0x7fffffff};
            if (on) best = (ValIdx){(e2 / s2) / cq[lane], cidx[lane]};
#define CSM_ARG_STEP(o) { ValIdx y; y.v = lane_xor<o>(best.v); y.i = lane_xor<o>(best.i); best = vi_max(best, y); }
            CSM_ARG_STEP(32) CSM_ARG_STEP(16) CSM_ARG_STEP(8) CSM_ARG_STEP(4) CSM_ARG_STEP(2) CSM_ARG_STEP(1)
#undef CSM_ARG_STEP
            if (lane == 0) {
                out[row] = best.i;
                if constexpr (Params::PENALTY) prm.wrote(row, pframe, best.i);
            }
        }
        STAMP(6);
        STAMP_FLUSH(300);
        return;
    }
    if constexpr (Params::TYPICAL) {
        if (typical_done) {                                 // (block-uniform) T need not hold the largest value: the max over T
            tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < NPT; ++j)
                if (threadIdx.x + 256 * j < V && key[j] >= prefix) tmax = fmaxf(tmax, val[j]);
        }
    }
    const float top = block_max(tmax, fred);
    // log_softmax over kept values, then softmax of that (torch evaluates both)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < V && key[j] >= prefix) s += expf(val[j] - top);
    }
    s = block_sum(s, fred);
    const float logsum = logf(s);
    const float ymax = (top - top) - logsum;
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < V && key[j] >= prefix) s2 += expf(((val[j] - top) - logsum) - ymax);
    }
    s2 = block_sum(s2, fred);
    STAMP(4);
    ValIdx best = {-INFINITY, 0x7fffffff};
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < V) {
            float p = 0.f;
            if (key[j] >= prefix) p = expf(((val[j] - top) - logsum) - ymax) / s2;
            best = vi_max(best, (ValIdx){p / qv[j], c});
        }
    }
    STAMP(5);
    best = block_arg<true>(best, red);
    if (threadIdx.x == 0) {
        out[row] = best.i;
        if constexpr (Params::PENALTY) prm.wrote(row, pframe, best.i);
    }
    STAMP(6);
    STAMP_FLUSH(300);
}

// Mimi split RVQ encode (moshi 0.2.2; call site reference src/csm/generator.py:117).  One block per frame; the
// residual lives in registers (4 floats per lane, replicated per wave); each wave scans C/4 codewords with
// coalesced 1-KiB row reads; squared L2 in fp32; the lowest index wins ties.
template <int D>
__global__ __launch_bounds__(256) void rvq_encode_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                         long long* __restrict__ codes, int T, int K, int C, int n_sem) {
    __shared__ ValIdx red[4];
    constexpr int PL = D / 64;
    const int t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float r[PL];
    for (int k = 0; k < K; ++k) {
        if (k == 0 || k == n_sem) {
#pragma unroll
            for (int j = 0; j < PL; ++j) r[j] = x[(size_t)t * D + lane + 64 * j];
        }
        const float* book = cb + (size_t)k * C * D;
        ValIdx best = {INFINITY, 0x7fffffff};
        for (int c = wave; c < C; c += 4) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < PL; ++j) {
                const float e = r[j] - book[(size_t)c * D + lane + 64 * j];
                d += e * e;
            }
            d = wave_sum(d);
            best = vi_min(best, (ValIdx){d, c});
        }
        best = block_arg<false>(best, red);
        if (threadIdx.x == 0) codes[(size_t)k * T + t] = best.i;
#pragma unroll
        for (int j = 0; j < PL; ++j) r[j] -= book[(size_t)best.i * D + lane + 64 * j];
    }
}

// codes [K][T] -> out[t][:] = sum_k cb[k][codes[k][t]] (ascending k, fp32)
__global__ __launch_bounds__(256) void rvq_decode_kernel(const long long* __restrict__ codes, const float* __restrict__ cb,
                                                         float* __restrict__ out, int T, int K, int C, int D) {
    const int t = blockIdx.x;
    for (int col = threadIdx.x; col < D; col += blockDim.x) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) {
            // a language model's audio vocabulary can be larger than the codebooks (CSM: 2051 ids, 2048 entries), so a sampled id
            // may lie outside them: bound it instead of reading past the table (ids inside [0, C) are untouched)
            long long c = codes[(size_t)k * T + t];
            c = c < 0 ? 0 : (c >= C ? C - 1 : c);
            acc += cb[((size_t)k * C + c) * D + col];
        }
        out[(size_t)t * D + col] = acc;
    }
}

}  // namespace

// The five samplers' launch: the kernel with 9 values per thread where the row fits, else SMP_PER_THREAD; one workgroup per row.
template <class Params>
static int sample_launch(const char* name, const float* logits, const float* q, int* out, int rows, int V, int ldl,
                         hipStream_t stream, const Params& prm) {
    CSM_REQUIRE(V <= 256 * SMP_PER_THREAD, "%s: V=%d exceeds %d", name, V, 256 * SMP_PER_THREAD);
    if (V <= 256 * 9) hipLaunchKernelGGL((sample_topk_kernel<9, Params>), dim3(rows), dim3(256), 0, stream, logits, q, out, V, ldl, prm);
    else hipLaunchKernelGGL((sample_topk_kernel<SMP_PER_THREAD, Params>), dim3(rows), dim3(256), 0, stream, logits, q, out, V, ldl, prm);
    CSM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int csm_sample_topk(const float* logits, const float* q, int* out, int rows, int V, int ldl, int topk,
                               float temperature, hipStream_t stream) {
    CSM_REQUIRE(logits && q && out && rows > 0 && V > 0 && ldl >= V, "csm_sample_topk: bad arguments");
    CSM_REQUIRE(topk > 0 && topk <= V && temperature > 0.f, "csm_sample_topk: bad topk=%d / temperature=%f", topk, temperature);
    return sample_launch("csm_sample_topk", logits, q, out, rows, V, ldl, stream, SampleScalars{topk, temperature});
}

extern "C" int csm_sample_topk_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                                    const float* temperature, hipStream_t stream) {
    CSM_REQUIRE(logits && q && out && topk && temperature && rows > 0 && V > 0 && ldl >= V, "csm_sample_topk_rows: bad arguments");
    return sample_launch("csm_sample_topk_rows", logits, q, out, rows, V, ldl, stream, SampleRows{topk, temperature});
}

extern "C" int csm_sample_filtered_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                                        const float* temperature, const float* top_p, const float* min_p, hipStream_t stream) {
    CSM_REQUIRE(logits && q && out && topk && temperature && top_p && min_p && rows > 0 && V > 0 && ldl >= V,
                "csm_sample_filtered_rows: bad arguments");
    return sample_launch("csm_sample_filtered_rows", logits, q, out, rows, V, ldl, stream,
                         SampleFiltered{topk, temperature, top_p, min_p});
}

extern "C" int csm_sample_processed_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                                         const float* temperature, const float* top_p, const float* min_p, const float* penalty,
                                         const int* window, int* hist, int ldh, int* frame, const int* live, int advance,
                                         hipStream_t stream) {
    CSM_REQUIRE(logits && q && out && topk && temperature && top_p && min_p && penalty && window && hist && frame && live &&
                rows > 0 && V > 0 && ldl >= V, "csm_sample_processed_rows: bad arguments");
    CSM_REQUIRE(ldh >= SMP_HIST, "csm_sample_processed_rows: ldh=%d is below the ring's %d", ldh, SMP_HIST);
    return sample_launch("csm_sample_processed_rows", logits, q, out, rows, V, ldl, stream,
                         SampleProcessed{topk, temperature, top_p, min_p, penalty, window, hist, ldh, frame, live, advance});
}

extern "C" int csm_sample_typical_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                                       const float* temperature, const float* top_p, const float* min_p, const float* penalty,
                                       const int* window, int* hist, int ldh, int* frame, const int* live, int advance,
                                       const float* typical_p, hipStream_t stream) {
    CSM_REQUIRE(logits && q && out && topk && temperature && top_p && min_p && penalty && window && hist && frame && live &&
                typical_p && rows > 0 && V > 0 && ldl >= V, "csm_sample_typical_rows: bad arguments");
    CSM_REQUIRE(ldh >= SMP_HIST, "csm_sample_typical_rows: ldh=%d is below the ring's %d", ldh, SMP_HIST);
    return sample_launch("csm_sample_typical_rows", logits, q, out, rows, V, ldl, stream,
                         SampleTypical{topk, temperature, top_p, min_p, penalty, window, hist, ldh, frame, live, advance, typical_p});
}

// What the model itself thought of a drawn code (csm_sample_stats_rows): the log-probability of codes[row], the entropy and the
// largest probability of softmax(logits[row]) - temperature 1, no filter, no penalty: the distribution every sampler knob acts
// on, and the likelihood the next-frame training objective sums.  One workgroup per row; the row is held in registers as the
// sampler holds it (thread t owns columns t + 256 j), so memory is read once.  With m = max x, d_i = x_i - m, e_i = expf(d_i):
//   S = sum e_i,  A = sum e_i d_i;   logprob = (x_code - m) - ln S,  entropy = ln S - A / S,  pmax = 1 / S.
// Order of every sum: a thread's columns ascending (j = 0, 1, ..), the wave butterfly of wave_sum / wave_max, then the four wave
// partials from LDS in wave order - no atomics, nothing depends on gridDim: a row's bits are the same alone and among 511 others.
// The drawn code's logit is picked out of the registers by the thread that owns its column (a compare per slot, no dynamic
// index: no scratch); that thread writes logprob.  A code outside [0, V) has no owner: thread 0 writes -inf.  A column at -inf
// has e = 0 and adds nothing to A (the limit of e d, not the NaN of 0 * inf).
namespace {
template <int NPT>
__global__ __launch_bounds__(256) void sample_stats_kernel(const float* __restrict__ logits, const int* __restrict__ codes,
                                                           float* __restrict__ logprob, float* __restrict__ entropy,
                                                           float* __restrict__ pmax, int V, int ldl) {
    __shared__ float red[3][4];
    const int row = blockIdx.x;
    const float* x = logits + (size_t)row * ldl;
    const int code = codes[row];                            // (block-uniform, in flight with the row)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float val[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = threadIdx.x + 256 * j;
        val[j] = c < V ? x[c] : -INFINITY;
    }
    float tmax = val[0], xc = 0.f;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        tmax = fmaxf(tmax, val[j]);
        if (threadIdx.x + 256 * j == code) xc = val[j];
    }
    tmax = wave_max(tmax);
    if (lane == 0) red[0][w] = tmax;
    __syncthreads();
    const float m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    float s = 0.f, a = 0.f;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        if (threadIdx.x + 256 * j < V) {
            const float d = val[j] - m;
            const float e = expf(d);
            s += e;
            if (e > 0.f) a += e * d;
        }
    }
    s = wave_sum(s);
    a = wave_sum(a);
    if (lane == 0) { red[1][w] = s; red[2][w] = a; }
    __syncthreads();
    const float S = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    const float A = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    const float lnS = logf(S);
    const bool inside = (unsigned)code < (unsigned)V;
    if (logprob) {
        if (inside && (code & 255) == (int)threadIdx.x) logprob[row] = (xc - m) - lnS;
        if (!inside && threadIdx.x == 0) logprob[row] = -INFINITY;
    }
    if (threadIdx.x == 0) {
        if (entropy) entropy[row] = lnS - A / S;
        if (pmax) pmax[row] = 1.f / S;
    }
}
}  // namespace

extern "C" int csm_sample_stats_rows(const float* logits, const int* codes, float* logprob, float* entropy, float* pmax,
                                     int rows, int V, int ldl, hipStream_t stream) {
    CSM_REQUIRE(logits && codes, "csm_sample_stats_rows: null logits or codes");
    CSM_REQUIRE(logprob || entropy || pmax, "csm_sample_stats_rows: no output (logprob, entropy and pmax are all null)");
    CSM_REQUIRE(rows > 0, "csm_sample_stats_rows: rows=%d must be positive", rows);
    CSM_REQUIRE(V > 0 && V <= 256 * SMP_PER_THREAD, "csm_sample_stats_rows: V=%d outside 1..%d", V, 256 * SMP_PER_THREAD);
    CSM_REQUIRE(ldl >= V, "csm_sample_stats_rows: ldl=%d is below V=%d", ldl, V);
    CSM_REQUIRE(((uintptr_t)logits | (uintptr_t)codes | (uintptr_t)logprob | (uintptr_t)entropy | (uintptr_t)pmax) % 4 == 0,
                "csm_sample_stats_rows: a pointer is not 4-byte aligned");
    if (V <= 256 * 9) hipLaunchKernelGGL((sample_stats_kernel<9>), dim3(rows), dim3(256), 0, stream, logits, codes, logprob, entropy, pmax, V, ldl);
    else hipLaunchKernelGGL((sample_stats_kernel<SMP_PER_THREAD>), dim3(rows), dim3(256), 0, stream, logits, codes, logprob, entropy, pmax, V, ldl);
    CSM_CHECK_LAUNCH("csm_sample_stats_rows");
    return 0;
}

extern "C" int csm_rvq_encode(const float* x, const float* codebooks, long long* codes, int T, int K, int C, int D,
                              int n_semantic, hipStream_t stream) {
    CSM_REQUIRE(x && codebooks && codes && T > 0 && K > 0 && C > 0, "csm_rvq_encode: bad arguments");
    CSM_REQUIRE(D == 256 || D == 128 || D == 64, "csm_rvq_encode: codebook dim %d unsupported (64/128/256)", D);
    CSM_REQUIRE(n_semantic >= 0 && n_semantic <= K, "csm_rvq_encode: n_semantic out of range");
#define L(DD) hipLaunchKernelGGL((rvq_encode_kernel<DD>), dim3(T), dim3(256), 0, stream, x, codebooks, codes, T, K, C, n_semantic)
    if (D == 256) L(256); else if (D == 128) L(128); else L(64);
#undef L
    CSM_CHECK_LAUNCH("csm_rvq_encode");
    return 0;
}

extern "C" int csm_rvq_decode(const long long* codes, const float* codebooks, float* out, int T, int K, int C, int D,
                              hipStream_t stream) {
    CSM_REQUIRE(codes && codebooks && out && T > 0 && K > 0 && C > 0 && D > 0, "csm_rvq_decode: bad arguments");
    hipLaunchKernelGGL(rvq_decode_kernel, dim3(T), dim3(256), 0, stream, codes, codebooks, out, T, K, C, D);
    CSM_CHECK_LAUNCH("csm_rvq_decode");
    return 0;
}

// ================================================================================================ batch-1 decode path
// Reference Model.generate_frame (src/csm/models/model.py:140-195) runs one backbone position and 31 decoder positions
// per 80-ms frame against KV caches: every projection is a matrix-VECTOR product bound by weight streaming
// (1.95 GB + 31 x 0.22 GB of bf16 weights per frame), attention is a cache read.  These kernels keep the weights'
// [N][K] layout, load 16 B per lane straight to registers (an LDS round trip is pure overhead when nothing is shared
// between waves) and reduce with wave shuffles.
namespace {

// (the K-extension of these products - GemvExt, GemvExtRows, ExtKind, ext_load / ext_fma / ext_dot - is gemv_ext.h: quant.hip's
//  FP8 families take the same packs; the B = 5..16 product, gemv_mfma_kernel and its launcher, is gemv_mfma.h: one kernel for both
//  weight formats)

// y[b][n] = sum_k x[b][k] * W[n][k] (+ R[b][n]);  one wave per output row, NB <= 4 batch rows share every weight load.
// Two optional fusions remove the tiny kernels that otherwise sit between the matrix-vector products of a decode step:
//   norm_w != NULL : x is RMS-normalised on its way into LDS (same arithmetic and summation order as rmsnorm_fwd_kernel:
//                    one wave per row, lane-strided chunks, wave_sum, one rounding of x * rstd * w to bf16);
//   SWIGLU         : W holds gate/up rows interleaved (w13); a wave computes rows 2i and 2i+1 and writes
//                    y[b][i] = silu(g) * u with g, u rounded to bf16 first (what swiglu_fwd_kernel reads back);
//   row_index      : batch row b of x is row (row_index[b] + row_offset) of a table (the embedding of a sampled code).
template <int NB, typename OutT, bool SWIGLU, typename... Ext>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W, OutT* __restrict__ y,
                                                   const bf16_t* __restrict__ R, int N, int K, int ldw, int ldx, int ldy,
                                                   const bf16_t* __restrict__ norm_w, float eps, const int* __restrict__ row_index,
                                                   int row_offset, Ext... ext) {
    constexpr int EK = ExtKind<Ext...>::v;
    constexpr bool EXT = EK == 1;
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem_x);            // [NB][K]
    __shared__ float rs[4];
    for (int i = threadIdx.x * 8; i < NB * K; i += blockDim.x * 8) {
        const int b = i / K, k = i - b * K;
        const size_t row = row_index ? (size_t)(row_index[b] + row_offset) : (size_t)b;   // x = table[index[b] + offset]: embedding lookup
        *reinterpret_cast<U4*>(xs + i) = *reinterpret_cast<const U4*>(x + row * ldx + k);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    if (norm_w) {
        const int wv = threadIdx.x >> 6;
        if (wv < NB) {
            float ss = 0.f;
            for (int c = lane; c < (K >> 3); c += 64) {
                float f[8];
                unpack8(*reinterpret_cast<const U4*>(xs + wv * K + c * 8), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
            }
            ss = wave_sum(ss);
            if (lane == 0) rs[wv] = rsqrtf(ss / (float)K + eps);
        }
        __syncthreads();
        for (int i = threadIdx.x * 8; i < NB * K; i += blockDim.x * 8) {
            const int b = i / K, k = i - b * K;
            float f[8], w8[8];
            unpack8(*reinterpret_cast<const U4*>(xs + i), f);
            unpack8(*reinterpret_cast<const U4*>(norm_w + k), w8);
            const float r = rs[b];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = f[j] * r * w8[j];
            *reinterpret_cast<U4*>(xs + i) = pack8(f);
        }
        __syncthreads();
    }
    constexpr int RW = SWIGLU ? 2 : 1;                          // weight rows per output
    const int NO = N / RW;
    for (int n = blockIdx.x * wpb + (threadIdx.x >> 6); n < NO; n += gridDim.x * wpb) {
        float acc[RW][NB];
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
        const bf16_t* w = W + (size_t)n * RW * ldw;
        for (int k = lane * 8; k < K; k += 512) {
            float wf[RW][8];
#pragma unroll
            for (int r = 0; r < RW; ++r) unpack8(*reinterpret_cast<const U4*>(w + (size_t)r * ldw + k), wf[r]);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                float xf[8];
                unpack8(*reinterpret_cast<const U4*>(xs + b * K + k), xf);
#pragma unroll
                for (int r = 0; r < RW; ++r)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[r][b] += wf[r][j] * xf[j];
            }
        }
        float bias[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) bias[r] = 0.f;
        if constexpr (EXT) {
            __builtin_amdgcn_sched_barrier(0);                // (the extension's loads stay behind the main products: registers)
            const GemvExt& e = ext_arg(ext...);
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const U4 eb = ext_load(e.Bx + (size_t)(n * RW + r) * e.ldb, lane, e.kx);
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[r][b] = ext_fma(acc[r][b], eb, ext_load(e.t + (size_t)b * e.ldt, lane, e.kx));
                if (e.bias) bias[r] = bf2f(e.bias[n * RW + r]);
            }
        }
        float rbias[RW][NB];                                  // (GemvExtRows: each row's own adapter)
        bool ron[NB];
        if constexpr (EK == 2) {
            __builtin_amdgcn_sched_barrier(0);
            const GemvExtRows& e = ext_rows_arg(ext...);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int a = ext_row_adapter(e, b);
                ron[b] = a >= 0;
#pragma unroll
                for (int r = 0; r < RW; ++r) rbias[r][b] = 0.f;
                if (a >= 0) {
                    const U4 tb = ext_load(e.t + (size_t)b * e.ldt, lane, e.kx);
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
                        acc[r][b] = ext_fma(acc[r][b], ext_load(e.Bx[a] + (size_t)(n * RW + r) * e.ldb, lane, e.kx), tb);
                        rbias[r][b] = ext_row_bias(e, a, n * RW + r);
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float v = wave_sum(acc[0][b]);
            if constexpr (EXT) v += bias[0];
            if constexpr (EK == 2) { if (ron[b]) v += rbias[0][b]; }
            if constexpr (SWIGLU) {
                float us = wave_sum(acc[1][b]);
                if constexpr (EXT) us += bias[1];
                if constexpr (EK == 2) { if (ron[b]) us += rbias[1][b]; }
                const float g = bf2f(f2bf(v)), u = bf2f(f2bf(us));
                v = silu(g) * u;
            }
            if (lane == 0) {
                if (R) v += bf2f(R[(size_t)b * ldy + n]);
                if constexpr (sizeof(OutT) == 2) y[(size_t)b * ldy + n] = f2bf(v);
                else y[(size_t)b * ldy + n] = v;
            }
        }
    }
}

// The same product for ONE batch row with x held in REGISTERS by every wave (round 4): K = 512 KCH, lane l owns the chunks
// k = 8 l + 512 c, c < KCH - the very chunks it multiplies in gemv_kernel's loop - so the whole of x is in the wave (KCH 16-byte
// loads per lane, L2 hits) and the RMSNorm prologue is a wave reduction: no LDS copy of x, no workgroup barrier (gemv_kernel has
// three in front of its first weight load), and the wave's weight rows are requested before anything else.  Same arithmetic
// in the same order as gemv_kernel<1, ...> (bit-identical: tests/test_e2e_gpu.py decode checks).  NT: non-temporal weight loads
// for matrices that are streamed once per frame (the backbone's 1.9 GB), so that they do not push the depth decoder's 222 MB -
// re-read 31 times per frame - out of the Infinity Cache.
// RPW (round 4): outputs per wave.  The w13 product of the depth decoder (K = 1024, 8192 gate/up pairs, 32 MB) runs one pair per
// wave; two and four pairs per wave (one normalisation of x per wave instead of per pair) were measured at 207.5 / 204 against
// 207.5 frames/s - the launch is bound by its weight stream - so 1 stays the default (csm_set_decode_tuning(2, n)).  A pair's two
// row sums share one butterfly: v_permlane32_swap(gate, up) leaves the gate partials in lanes 0-31 and the up partials in lanes
// 32-63, the remaining xor-16 .. xor-1 steps never cross the halves - the same additions as two separate wave_sum() calls, so the
// same bits.
template <int KCH, typename OutT, bool SWIGLU, bool NT, int RPW = 1, typename... Ext>
__global__ __launch_bounds__(256) void gemv_reg_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W, OutT* __restrict__ y,
                                                       const bf16_t* __restrict__ R, int N, int ldw, int ldx, int ldy,
                                                       const bf16_t* __restrict__ norm_w, float eps, const int* __restrict__ row_index,
                                                       int row_offset, Ext... ext) {
    constexpr int EK = ExtKind<Ext...>::v;
    constexpr bool EXT = EK == 1;
    constexpr int K = 512 * KCH;
    constexpr int RW = SWIGLU ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int n0 =(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW;
    const int NO = N / RW;
    if (n0 >= NO) return;
    STAMP_DECL;
    STAMP(0);
    // the wave's weight rows: requested first (outputs past the end re-read the last one and are never stored)
    U4 wq[RPW][RW][KCH];
#pragma unroll
    for (int o = 0; o < RPW; ++o) {
        const bf16_t* w = W + (size_t)min(n0 + o, NO - 1) * RW * ldw + lane * 8;
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int c = 0; c < KCH; ++c) {
                const U4* p = reinterpret_cast<const U4*>(w + (size_t)r * ldw + 512 * c);
                wq[o][r][c] = NT ? __builtin_nontemporal_load(p) : *p;
            }
    }
    const size_t row = row_index ? (size_t)(row_index[0] + row_offset) : (size_t)0;
    U4 xq[KCH];
#pragma unroll
    for (int c = 0; c < KCH; ++c) xq[c] = *reinterpret_cast<const U4*>(x + row * ldx + lane * 8 + 512 * c);
#ifdef CSM_DECODE_STAMPS
    STAMP(1);
#pragma unroll
    for (int c = 0; c < KCH; ++c) asm volatile("" : "+v"(xq[c].x), "+v"(xq[c].y), "+v"(xq[c].z), "+v"(xq[c].w));     // x has arrived
    STAMP(2);
#pragma unroll
    for (int o = 0; o < RPW; ++o)
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int c = 0; c < KCH; ++c) asm volatile("" : "+v"(wq[o][r][c].x), "+v"(wq[o][r][c].y), "+v"(wq[o][r][c].z), "+v"(wq[o][r][c].w));   // weights have arrived
    STAMP(3);
#endif
    if (norm_w) {
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            float f[8];
            unpack8(xq[c], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
        }
        ss = wave_sum(ss);
        const float rs = rsqrtf(ss / (float)K + eps);
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            float f[8], w8[8];
            unpack8(xq[c], f);
            unpack8(*reinterpret_cast<const U4*>(norm_w + lane * 8 + 512 * c), w8);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = f[j] * rs * w8[j];
            xq[c] = pack8(f);
        }
    }
    float acc[RPW][RW];
#pragma unroll
    for (int o = 0; o < RPW; ++o)
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[o][r] = 0.f;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
        float xf[8];
        unpack8(xq[c], xf);
#pragma unroll
        for (int o = 0; o < RPW; ++o)
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                float wf[8];
                unpack8(wq[o][r][c], wf);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[o][r] += wf[j] * xf[j];
            }
    }
    STAMP(4);
    float bias[RPW][RW];
#pragma unroll
    for (int o = 0; o < RPW; ++o)
#pragma unroll
        for (int r = 0; r < RW; ++r) bias[o][r] = 0.f;
    if constexpr (EXT) {
        __builtin_amdgcn_sched_barrier(0);                    // (the extension's loads stay behind the main products: registers)
        const GemvExt& e = ext_arg(ext...);
        const U4 et = ext_load(e.t, lane, e.kx);
#pragma unroll
        for (int o = 0; o < RPW; ++o)
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                acc[o][r] = ext_fma(acc[o][r], ext_load(e.Bx + (size_t)(min(n0 + o, NO - 1) * RW + r) * e.ldb, lane, e.kx), et);
                if (e.bias) bias[o][r] = bf2f(e.bias[min(n0 + o, NO - 1) * RW + r]);
            }
    }
    bool ron = false;                                         // (GemvExtRows: the one row's own adapter)
    if constexpr (EK == 2) {
        __builtin_amdgcn_sched_barrier(0);
        const GemvExtRows& e = ext_rows_arg(ext...);
        const int a = ext_row_adapter(e, 0);
        ron = a >= 0;
        if (ron) {
            const U4 et = ext_load(e.t, lane, e.kx);
#pragma unroll
            for (int o = 0; o < RPW; ++o)
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    acc[o][r] = ext_fma(acc[o][r], ext_load(e.Bx[a] + (size_t)(min(n0 + o, NO - 1) * RW + r) * e.ldb, lane, e.kx), et);
                    bias[o][r] = ext_row_bias(e, a, min(n0 + o, NO - 1) * RW + r);
                }
        }
    }
#pragma unroll
    for (int o = 0; o < RPW; ++o) {
        float v;
        if constexpr (SWIGLU) {
            float gs, us;
            wave_sum2(acc[o][0], acc[o][1], gs, us);             // both row sums in one butterfly
            if constexpr (EXT) { gs += bias[o][0]; us += bias[o][1]; }
            if constexpr (EK == 2) { if (ron) { gs += bias[o][0]; us += bias[o][1]; } }
            const float g = bf2f(f2bf(gs)), u = bf2f(f2bf(us));
            v = silu(g) * u;
        } else {
            v = wave_sum(acc[o][0]);
            if constexpr (EXT) v += bias[o][0];
            if constexpr (EK == 2) { if (ron) v += bias[o][0]; }
        }
        if (lane == 0 && n0 + o < NO) {
            if (R) v += bf2f(R[n0 + o]);
            if constexpr (sizeof(OutT) == 2) y[n0 + o] = f2bf(v);
            else y[n0 + o] = v;
        }
    }
    STAMP(5);
    STAMP_FLUSH(100 + KCH * 4 + (SWIGLU ? 2 : 0) + (norm_w ? 1 : 0));
}

// Two to four batch rows with x in registers (round 4; generate_batch): wave b of a workgroup prepares row b of x (RMSNorm as a
// wave reduction, rounded to bf16 exactly as gemv_kernel leaves it in LDS) and publishes it as fp32 behind ONE barrier; every wave
// then keeps ALL rows of the elements it multiplies in registers, so a weight chunk is unpacked once and feeds NB fused
// multiply-adds per element, two rows per v_pk_fma_f32 - 24 instructions per 16 bytes of weights at NB = 4, what one row costs -
// instead of re-reading and re-unpacking every row's x from LDS behind three barriers (gemv_kernel<4>: 8.5 us where the one-row
// kernel takes 4.6).  (Every wave preparing all rows itself - no LDS, no barrier - was slower than gemv_kernel: 419 against 439
// frames/s aggregate at B = 4; the preparation is ~130 instructions per row, the products of a K = 1024 row only ~50.)  K = 1024 /
// 2048; K = 8192 stays with gemv_kernel.  Every (row, output) accumulator sees gemv_kernel's products in gemv_kernel's order:
// bit-identical per row to the one-row kernels (test_batched_matrix_vector_kernels_match_single_row).
typedef float csm_f2 __attribute__((ext_vector_type(2)));
// SC = chunks per segment: K = 8192 (KCH = 16) walks x in four segments of four chunks (the fp32 rows stay in LDS, 128 KB at four
// rows; a segment's elements are in registers while its weight chunks are multiplied), K <= 2048 is one segment.
template <int KCH, int NB, typename OutT, bool SWIGLU, bool NT, int SC = KCH, typename... Ext>
__global__ __launch_bounds__(256) void gemv_regn_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W, OutT* __restrict__ y,
                                                        const bf16_t* __restrict__ R, int N, int ldw, int ldx, int ldy,
                                                        const bf16_t* __restrict__ norm_w, float eps, const int* __restrict__ row_index,
                                                        int row_offset, Ext... ext) {
    constexpr int EK = ExtKind<Ext...>::v;
    constexpr bool EXT = EK == 1;
    constexpr int K = 512 * KCH;
    constexpr int RW = SWIGLU ? 2 : 1;
    constexpr int NP = (NB + 1) / 2;                                        // row pairs (the last one half empty for odd NB)
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int NO = N / RW;
    const bool live = n < NO;                              // (every wave reaches the barrier; rows past the end re-read the last one)
    U4 wq[RW][KCH];
    const bf16_t* w = W + (size_t)(live ? n : NO - 1) * RW * ldw + lane * 8;
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            const U4* p = reinterpret_cast<const U4*>(w + (size_t)r * ldw + 512 * c);
            wq[r][c] = NT ? __builtin_nontemporal_load(p) : *p;
        }
    // wave b < NB prepares row b of x (RMSNorm as a wave reduction, rounded to bf16 as gemv_kernel's LDS copy is) and publishes it
    // as fp32; ONE barrier; every lane then takes the elements it multiplies, two rows per register pair
    extern __shared__ __attribute__((aligned(16))) char smem_n[];
    float (*xsh)[K] = reinterpret_cast<float (*)[K]>(smem_n);                // [NB][K]
    const int wv = threadIdx.x >> 6;
    if (wv < NB) {
        const int b = wv;
        const size_t row = row_index ? (size_t)(row_index[b] + row_offset) : (size_t)b;
        U4 xr[KCH];
#pragma unroll
        for (int c = 0; c < KCH; ++c) xr[c] = *reinterpret_cast<const U4*>(x + row * ldx + lane * 8 + 512 * c);
        float rsn = 1.f;
        if (norm_w) {
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < KCH; ++c) {
                float f[8];
                unpack8(xr[c], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
            }
            ss = wave_sum(ss);
            rsn = rsqrtf(ss / (float)K + eps);
        }
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            float f[8];
            unpack8(xr[c], f);
            if (norm_w) {
                float w8[8];
                unpack8(*reinterpret_cast<const U4*>(norm_w + lane * 8 + 512 * c), w8);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = f[j] * rsn * w8[j];
                unpack8(pack8(f), f);                                        // the bf16 rounding gemv_kernel's LDS copy carries
            }
            *reinterpret_cast<float4*>(&xsh[b][lane * 8 + 512 * c]) = make_float4(f[0], f[1], f[2], f[3]);
            *reinterpret_cast<float4*>(&xsh[b][lane * 8 + 512 * c + 4]) = make_float4(f[4], f[5], f[6], f[7]);
        }
    }
    lds_barrier();                                                           // (LDS only: the weight rows stay in flight)
    csm_f2 acc[RW][NP];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int q = 0; q < NP; ++q) acc[r][q] = (csm_f2){0.f, 0.f};
    static_assert(KCH % SC == 0, "whole segments");
#pragma unroll
    for (int sg = 0; sg < KCH / SC; ++sg) {
        csm_f2 xp[NP][SC][8];                                                // (row 2p, row 2p+1) of the segment's elements this lane multiplies
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int cc = 0; cc < SC; ++cc) {
                const int c = sg * SC + cc;
                const float4 a0 = *reinterpret_cast<const float4*>(&xsh[2 * q][lane * 8 + 512 * c]);
                const float4 a1 = *reinterpret_cast<const float4*>(&xsh[2 * q][lane * 8 + 512 * c + 4]);
                float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
                if (2 * q + 1 < NB) {
                    b0 = *reinterpret_cast<const float4*>(&xsh[2 * q + 1][lane * 8 + 512 * c]);
                    b1 = *reinterpret_cast<const float4*>(&xsh[2 * q + 1][lane * 8 + 512 * c + 4]);
                }
                xp[q][cc][0] = (csm_f2){a0.x, b0.x}; xp[q][cc][1] = (csm_f2){a0.y, b0.y}; xp[q][cc][2] = (csm_f2){a0.z, b0.z}; xp[q][cc][3] = (csm_f2){a0.w, b0.w};
                xp[q][cc][4] = (csm_f2){a1.x, b1.x}; xp[q][cc][5] = (csm_f2){a1.y, b1.y}; xp[q][cc][6] = (csm_f2){a1.z, b1.z}; xp[q][cc][7] = (csm_f2){a1.w, b1.w};
            }
#pragma unroll
        for (int cc = 0; cc < SC; ++cc) {
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                float wf[8];
                unpack8(wq[r][sg * SC + cc], wf);
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int q = 0; q < NP; ++q) acc[r][q] = __builtin_elementwise_fma((csm_f2){wf[j], wf[j]}, xp[q][cc][j], acc[r][q]);
            }
        }
    }
    float bias[RW];
    U4 eb[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) bias[r] = 0.f;
    if constexpr (EXT) {
        __builtin_amdgcn_sched_barrier(0);                    // (the extension's loads stay behind the main products: registers)
        const GemvExt& e = ext_arg(ext...);
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            eb[r] = ext_load(e.Bx + (size_t)((live ? n : NO - 1) * RW + r) * e.ldb, lane, e.kx);
            if (e.bias) bias[r] = bf2f(e.bias[(live ? n : NO - 1) * RW + r]);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        float a0 = (b & 1) ? acc[0][b >> 1].y : acc[0][b >> 1].x;
        U4 et;
        if constexpr (EXT) { et = ext_load(ext_arg(ext...).t + (size_t)b * ext_arg(ext...).ldt, lane, ext_arg(ext...).kx); a0 = ext_fma(a0, eb[0], et); }
        // GemvExtRows: row b's own adapter - its Bx chunk and bias are loaded here, then the same ext_fma as GemvExt's
        bool ron = false;
        float rb[RW];
        if constexpr (EK == 2) {
            const GemvExtRows& e = ext_rows_arg(ext...);
            const int a = ext_row_adapter(e, b);
            ron = a >= 0;
            if (ron) {
                et = ext_load(e.t + (size_t)b * e.ldt, lane, e.kx);
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    eb[r] = ext_load(e.Bx[a] + (size_t)((live ? n : NO - 1) * RW + r) * e.ldb, lane, e.kx);
                    rb[r] = ext_row_bias(e, a, (live ? n : NO - 1) * RW + r);
                }
                a0 = ext_fma(a0, eb[0], et);
            }
        }
        float v;
        if constexpr (SWIGLU) {
            float a1 = (b & 1) ? acc[1][b >> 1].y : acc[1][b >> 1].x;
            if constexpr (EXT) a1 = ext_fma(a1, eb[1], et);
            if constexpr (EK == 2) { if (ron) a1 = ext_fma(a1, eb[1], et); }
            float gs, us;
            wave_sum2(a0, a1, gs, us);
            if constexpr (EXT) { gs += bias[0]; us += bias[1]; }
            if constexpr (EK == 2) { if (ron) { gs += rb[0]; us += rb[1]; } }
            const float g = bf2f(f2bf(gs)), u = bf2f(f2bf(us));
            v = silu(g) * u;
        } else {
            v = wave_sum(a0);
            if constexpr (EXT) v += bias[0];
            if constexpr (EK == 2) { if (ron) v += rb[0]; }
        }
        if (lane == 0 && live) {
            if (R) v += bf2f(R[(size_t)b * ldy + n]);
            if constexpr (sizeof(OutT) == 2) y[(size_t)b * ldy + n] = f2bf(v);
            else y[(size_t)b * ldy + n] = v;
        }
    }
}

// Five to sixteen batch rows (generate_batch at B > 4): gemv_mfma_kernel<WeightBf16, ...> of gemv_mfma.h - the MFMA product that the
// FP8 decode (quant.hip) instantiates with its own weight format.

// y[b][n] = sum_k x[b][k] * W[k][n]  (weights stored K-major, e.g. audio_head[i] = [d'][V]): a thread owns 8 columns.
template <int NB, typename OutT>
__global__ __launch_bounds__(256) void gemv_t_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W, OutT* __restrict__ y,
                                                     int N, int K, int ldw, int ldx, int ldy) {
    const int n0 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (n0 >= N) return;
    float acc[NB][8];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[b][j] = 0.f;
    for (int k = 0; k < K; ++k) {
        float wf[8];
        unpack8(*reinterpret_cast<const U4*>(W + (size_t)k * ldw + n0), wf);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float xv = bf2f(x[(size_t)b * ldx + k]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[b][j] += xv * wf[j];
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (n0 + j < N) {
                if constexpr (sizeof(OutT) == 2) y[(size_t)b * ldy + n0 + j] = f2bf(acc[b][j]);
                else y[(size_t)b * ldy + n0 + j] = acc[b][j];
            }
}

// copy the new position's K and V heads (already RoPE'd) from the fused qkv row into the caches [B][KV][S_max][HD]
__global__ __launch_bounds__(256) void kv_append_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                        const int* __restrict__ pos, int H, int KV, int HD, int S_max, int ld) {
    const int b = blockIdx.x;
    const int p = pos[b];
    const int per = KV * HD;
    for (int i = threadIdx.x * 8; i < per; i += blockDim.x * 8) {
        const int kvh = i / HD, d = i - kvh * HD;
        const size_t dst = (((size_t)b * KV + kvh) * S_max + p) * HD + d;
        *reinterpret_cast<U4*>(kc + dst) = *reinterpret_cast<const U4*>(qkv + (size_t)b * ld + H * HD + i);
        *reinterpret_cast<U4*>(vc + dst) = *reinterpret_cast<const U4*>(qkv + (size_t)b * ld + (H + KV) * HD + i);
    }
}

// A parked history [planes = layers * 2 * KV][len][HD] (K planes before V planes per layer) without its positions keep ..
// keep+drop-1: the head is copied, the tail moves `drop` positions down and its KEYS are rotated back by drop positions -
// row `drop` of the RoPE table with the sine negated (rope(k, p + d) -> rope(k, p): a context shift).  Out of place: a thread
// owns one 16-byte vector (4 interleaved pairs) of one position and walks the planes, so the table row is read once.
template <int HD>
__global__ __launch_bounds__(256) void kv_shift_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                       const float* __restrict__ trow, int planes, int KV, int len, int keep,
                                                       int drop) {
    constexpr int VPR = HD / 8;                                    // 16-byte vectors per position
    const int nl = len - drop;
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= (long long)nl * VPR) return;
    const int p = (int)(v / VPR), d8 = (int)(v - (long long)p * VPR);
    const bool tail = p >= keep;
    float c[4] = {1.f, 1.f, 1.f, 1.f}, sn[4] = {0.f, 0.f, 0.f, 0.f};
    if (tail) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = trow[(d8 * 4 + j) * 2]; sn[j] = trow[(d8 * 4 + j) * 2 + 1]; }
    }
    const size_t so = (size_t)(tail ? p + drop : p) * HD + d8 * 8, dof = (size_t)p * HD + d8 * 8;
    for (int hp = blockIdx.y; hp < planes; hp += gridDim.y) {      // hp = (layer * 2 + plane) * KV + kv head
        U4 u = *reinterpret_cast<const U4*>(src + (size_t)hp * len * HD + so);
        if (tail && ((hp / KV) & 1) == 0) {                        // a key of the tail
            float f[8];
            unpack8(u, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) rope_rot(f[2 * j], f[2 * j + 1], c[j], -sn[j]);
            u = pack8(f);
        }
        *reinterpret_cast<U4*>(dst + (size_t)hp * nl * HD + dof) = u;
    }
}

// The rows form of DecodeState.resume_row: R <= 16 parked histories [planes = layers * 2 * KV][len][HD] into rows of the cache
// allocation [layers][2][B][KV][S_max][HD], positions 0 .. len-1, and pos[row] = len - 1.  The table travels by value in the
// kernel arguments (as AppendRows does in attention.hip); several segments may name one source.  Grid x = the segments' chunks
// of 256 16-byte vectors of one plane: a workgroup finds its segment by walking the table with its block index (scalar work)
// and never straddles two.  For a fixed plane both sides are contiguous runs of len * HD elements, so consecutive lanes copy
// consecutive vectors; a thread walks the planes four at a time (four loads in flight, then four stores).  No LDS.
struct ForkRows {
    const bf16_t* src[16];   // parked history of the segment
    int row[16];             // batch row of the caches
    int len[16];             // positions (0 from R on)
};

template <int HD>
__global__ __launch_bounds__(256) void kv_fork_rows_kernel(ForkRows a, bf16_t* __restrict__ kv, int* __restrict__ pos, int planes,
                                                           int B, int KV, int S_max) {
    constexpr int VPR = HD / 8;                                    // 16-byte vectors per position
    int t = blockIdx.x, row = 0, len = 0, chunk = 0;
    const bf16_t* src = nullptr;
    bool found = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int nc = (a.len[r] * VPR + 255) >> 8;
        if (!found && t < nc) {
            src = a.src[r]; row = a.row[r]; len = a.len[r]; chunk = t;
            found = true;
        }
        if (!found) t -= nc;
    }
    if (!found) return;                                            // (the grid is exactly the chunks: not reached)
    if (chunk == 0 && blockIdx.y == 0 && threadIdx.x == 0) pos[row] = len - 1;
    const int v = chunk * 256 + threadIdx.x;
    if (v >= len * VPR) return;
    const int gy = gridDim.y;
    for (int hp = blockIdx.y; hp < planes; hp += 4 * gy) {         // hp = (layer * 2 + plane) * KV + kv head
        U4 u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (hp + j * gy < planes) u[j] = *reinterpret_cast<const U4*>(src + (size_t)(hp + j * gy) * len * HD + (size_t)v * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int h = hp + j * gy;
            if (h < planes) {
                const int lp = h / KV, kvh = h - lp * KV;
                *reinterpret_cast<U4*>(kv + (((size_t)lp * B + row) * KV + kvh) * S_max * HD + (size_t)v * 8) = u[j];
            }
        }
    }
}

// The mirror of kv_fork_rows_kernel, the rows form of DecodeState.park_row: positions 0 .. len-1 of R <= 16 rows of the cache
// allocation into R separate contiguous destinations [planes][len][HD].  The same table walk, the same chunks, the same four
// planes in flight per thread; the cache is only read, pos is not an argument.  No LDS.
struct ParkRows {
    bf16_t* dst[16];         // parked history of the segment
    int row[16];             // batch row of the caches
    int len[16];             // positions (0 from R on)
};

template <int HD>
__global__ __launch_bounds__(256) void kv_park_rows_kernel(ParkRows a, const bf16_t* __restrict__ kv, int planes, int B, int KV,
                                                           int S_max) {
    constexpr int VPR = HD / 8;                                    // 16-byte vectors per position
    int t = blockIdx.x, row = 0, len = 0, chunk = 0;
    bf16_t* dst = nullptr;
    bool found = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int nc = (a.len[r] * VPR + 255) >> 8;
        if (!found && t < nc) {
            dst = a.dst[r]; row = a.row[r]; len = a.len[r]; chunk = t;
            found = true;
        }
        if (!found) t -= nc;
    }
    if (!found) return;                                            // (the grid is exactly the chunks: not reached)
    const int v = chunk * 256 + threadIdx.x;
    if (v >= len * VPR) return;
    const int gy = gridDim.y;
    for (int hp = blockIdx.y; hp < planes; hp += 4 * gy) {         // hp = (layer * 2 + plane) * KV + kv head
        U4 u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int h = hp + j * gy;
            if (h < planes) {
                const int lp = h / KV, kvh = h - lp * KV;
                u[j] = *reinterpret_cast<const U4*>(kv + (((size_t)lp * B + row) * KV + kvh) * S_max * HD + (size_t)v * 8);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (hp + j * gy < planes) *reinterpret_cast<U4*>(dst + (size_t)(hp + j * gy) * len * HD + (size_t)v * 8) = u[j];
    }
}

// The rings of the processed / typical samplers, row by row: code_hist [B][K][SMP_HIST] and hist_frame [B] of the state against a
// packed buffer [R][K * SMP_HIST + 1] (a row's ring, then its counter).  Block r moves row a.row[r]; to_state picks the direction -
// towards the state only the named rows are written, towards the packed buffer nothing of the state is.  hist_live is no argument.
struct HistRows {
    int row[16];
};

__global__ __launch_bounds__(256) void sample_hist_move_rows_kernel(HistRows a, int* __restrict__ code_hist, int* __restrict__ hist_frame,
                                                                    int* __restrict__ packed, int K, int to_state) {
    const int r = blockIdx.x, row = a.row[r], n = K * SMP_HIST;
    int* ring = code_hist + (size_t)row * n;
    int* pk = packed + (size_t)r * (n + 1);
    if (to_state) {
        for (int i = threadIdx.x; i < n; i += 256) ring[i] = pk[i];
        if (threadIdx.x == 0) hist_frame[row] = pk[n];
    } else {
        for (int i = threadIdx.x; i < n; i += 256) pk[i] = ring[i];
        if (threadIdx.x == 0) pk[n] = hist_frame[row];
    }
}

// one query position against the cache: block per (b, q-head); the scores of all S_max <= 8192 keys live in LDS (the launcher sizes it).
// table != NULL fuses what used to be two more launches per layer: the new position's q and k heads are rotated here
// (torchtune RoPE on interleaved pairs, same arithmetic and bf16 rounding as rope_kernel), and the first q-head block of
// every kv group appends the rotated k and the v of the new position to the caches.  Every block takes the new key /
// value from the qkv row, not from the cache, so blocks of one group do not race with the appending block.
template <int HD>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                          bf16_t* __restrict__ vc, bf16_t* __restrict__ out,
                                                          const int* __restrict__ pos, int H, int KV, int S_max, int ld,
                                                          float scale, const float* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) char smem_a[];
    float* sc = reinterpret_cast<float*>(smem_a);                 // [S_max] scores, then probabilities
    float* red = sc + S_max;                                       // 16 floats
    float* part = red + 16;                                        // [4 waves][HD] partial outputs
    float* qs = part + 4 * HD;                                     // [HD] query (rotated), bf16-rounded values
    float* kn = qs + HD;                                           // [HD] new key (rotated)
    const int h = blockIdx.x, b = blockIdx.y;
    const int rep = H / KV, kvh = h / rep;
    const int p = pos[b];
    const int n = p + 1;                                           // keys 0 .. pos
    const bf16_t* q = qkv + (size_t)b * ld + h * HD;
    const bf16_t* knew = qkv + (size_t)b * ld + (H + kvh) * HD;
    const bf16_t* vnew = qkv + (size_t)b * ld + (H + KV + kvh) * HD;
    bf16_t* K = kc + ((size_t)b * KV + kvh) * S_max * HD;
    bf16_t* V = vc + ((size_t)b * KV + kvh) * S_max * HD;
    if (threadIdx.x < HD / 2) {
        const int i = threadIdx.x;
        float c = 1.f, sn = 0.f;
        if (table) { c = table[((size_t)p * (HD / 2) + i) * 2]; sn = table[((size_t)p * (HD / 2) + i) * 2 + 1]; }
        const float q0 = bf2f(q[2 * i]), q1 = bf2f(q[2 * i + 1]), k0 = bf2f(knew[2 * i]), k1 = bf2f(knew[2 * i + 1]);
        float q0r = q0, q1r = q1, k0r = k0, k1r = k1;
        rope_rot(q0r, q1r, c, sn);
        rope_rot(k0r, k1r, c, sn);
        const bf16_t rq0 = f2bf(q0r), rq1 = f2bf(q1r);
        const bf16_t rk0 = f2bf(k0r), rk1 = f2bf(k1r);
        qs[2 * i] = bf2f(rq0); qs[2 * i + 1] = bf2f(rq1);
        kn[2 * i] = bf2f(rk0); kn[2 * i + 1] = bf2f(rk1);
        if (table && h % rep == 0) {
            K[(size_t)p * HD + 2 * i] = rk0; K[(size_t)p * HD + 2 * i + 1] = rk1;
            V[(size_t)p * HD + 2 * i] = vnew[2 * i]; V[(size_t)p * HD + 2 * i + 1] = vnew[2 * i + 1];
        }
    }
    __syncthreads();
    float qf[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) qf[c] = qs[c];
    float mx = -INFINITY;
    for (int s = threadIdx.x; s < n; s += blockDim.x) {
        float d = 0.f;
        if (s == p) {
#pragma unroll
            for (int c = 0; c < HD; ++c) d += qf[c] * kn[c];
        } else {
#pragma unroll
            for (int c = 0; c < HD / 8; ++c) {
                float kf[8];
                unpack8(*reinterpret_cast<const U4*>(K + (size_t)s * HD + c * 8), kf);
#pragma unroll
                for (int j = 0; j < 8; ++j) d += qf[c * 8 + j] * kf[j];
            }
        }
        d *= scale;
        sc[s] = d;
        mx = fmaxf(mx, d);
    }
    mx = block_max(mx, red);
    float sum = 0.f;
    for (int s = threadIdx.x; s < n; s += blockDim.x) {
        const float p = __expf(sc[s] - mx);
        sc[s] = p;
        sum += p;
    }
    sum = block_sum(sum, red);
    __syncthreads();
    // out[d] = sum_s p[s] V[s][d]: lane = 8 consecutive d's of a (HD/8)-lane group, groups stride over keys
    constexpr int LPR = HD / 8;                                    // lanes per key row
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR, ngrp = blockDim.x / LPR;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = grp; s < n; s += ngrp) {
        float vf[8];
        unpack8(*reinterpret_cast<const U4*>((s == p ? vnew : V + (size_t)s * HD) + sub * 8), vf);
        const float p = sc[s];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += p * vf[j];
    }
    // reduce the ngrp partials: first inside a wave (groups of a wave differ in lane bits >= log2(LPR)), then across waves
    static_assert(LPR == 8 || LPR == 16, "head_dim 64 or 128");
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if constexpr (LPR == 8) acc[j] += lane_xor<8>(acc[j]);
        acc[j] += lane_xor<16>(acc[j]);
        acc[j] += lane_xor<32>(acc[j]);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < LPR)
#pragma unroll
        for (int j = 0; j < 8; ++j) part[wave * HD + lane * 8 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < HD) {
        float o = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) o += part[w * HD + threadIdx.x];
        out[(size_t)b * H * HD + h * HD + threadIdx.x] = f2bf(o / sum);
    }
}


// The depth decoder's attention folded into the prologue of its output-projection matrix-vector product (round 3): a decoder
// step sees at most 32 keys (one frame's codebooks), so the attention of ALL heads is a few thousand multiply-adds - cheaper to
// recompute in every workgroup of the following product than to launch on its own (124 launches per generated frame, each
// ~7.5 us of launch + ramp for ~0.3 us of work).  Every workgroup: rotates q and the new k (torchtune RoPE, interleaved pairs),
// computes softmax(q K^T / sqrt(HD)) V over cache rows 0 .. pos-1 plus the new key / value taken from the qkv row, writes
// the bf16 result into LDS as the product's input vector, then runs the usual row-per-wave product with the residual.
// Workgroup 0 also appends the rotated k and the v of the new position to the caches (the others never read that row).
// The arithmetic follows attn_decode_kernel operation for operation - the same products in the same order, the same
// reduction trees (scores: one key per lane, a serial dot over HD; sum: a 64-lane butterfly; P.V: 16 key groups of 8-column
// slices, groups summed ((g0+g1)+(g2+g3)) per quartet and the quartets left to right) - so a frame decoded through this
// kernel is bit-identical to one decoded through csm_attn_decode_rope + csm_gemv_bf16 (tests/test_e2e_gpu.py).
template <int NB, int HD>
__global__ __launch_bounds__(512) void gemv_attn_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                        const int* __restrict__ pos, const float* __restrict__ table,
                                                        const bf16_t* __restrict__ W, bf16_t* __restrict__ y,
                                                        const bf16_t* __restrict__ R, int N, int H, int KV, int S_max, int ldq,
                                                        int ldw, int ldy, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    const int K = H * HD;
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem_x);                         // [NB][K]   attention output = the product's input
    float* qs = reinterpret_cast<float*>(smem_x + (size_t)NB * K * 2);      // [NB][H][HD]  rotated q (bf16-rounded values)
    float* kn = qs + (size_t)NB * H * HD;                                   // [NB][KV][HD] rotated new k
    float* pw = kn + (size_t)NB * KV * HD;                                  // [waves][64] probabilities
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rep = H / KV;
    // the wave's first weight row: requested before the attention prologue (it depends on nothing here; round 4: behind the two
    // barriers below its latency was the tail of every one of the 128 launches per frame)
    constexpr int KCH = 2;                                                  // K = H * HD = 1024 in the depth decoder: 2 chunks per lane
    const int row0 = blockIdx.x * (int)(blockDim.x >> 6) + wave;
    const bool pre = (K == 512 * KCH) && row0 < N;
    U4 wq0[KCH] = {};
    if (pre) {
#pragma unroll
        for (int c = 0; c < KCH; ++c) wq0[c] = *reinterpret_cast<const U4*>(W + (size_t)row0 * ldw + lane * 8 + 512 * c);
    }
    // ---- RoPE of q (all heads) and of the new k (all kv heads); workgroup 0 appends k, v to the caches
    for (int it = threadIdx.x; it < NB * (H + KV) * (HD / 2); it += blockDim.x) {
        const int i = it % (HD / 2), hh = (it / (HD / 2)) % (H + KV), b = it / ((HD / 2) * (H + KV));
        const int p = pos[b];
        const float c = table[((size_t)p * (HD / 2) + i) * 2], sn = table[((size_t)p * (HD / 2) + i) * 2 + 1];
        const bf16_t* src = qkv + (size_t)b * ldq + hh * HD;                 // q heads, then k heads, contiguous in the fused row
        const float x0 = bf2f(src[2 * i]), x1 = bf2f(src[2 * i + 1]);
        float y0 = x0, y1 = x1;
        rope_rot(y0, y1, c, sn);
        const bf16_t r0 = f2bf(y0), r1 = f2bf(y1);
        if (hh < H) {
            qs[((size_t)b * H + hh) * HD + 2 * i] = bf2f(r0); qs[((size_t)b * H + hh) * HD + 2 * i + 1] = bf2f(r1);
        } else {
            const int kvh = hh - H;
            kn[((size_t)b * KV + kvh) * HD + 2 * i] = bf2f(r0); kn[((size_t)b * KV + kvh) * HD + 2 * i + 1] = bf2f(r1);
            if (blockIdx.x == 0) {
                const bf16_t* vnew = qkv + (size_t)b * ldq + (H + KV + kvh) * HD;
                const size_t dst = (((size_t)b * KV + kvh) * S_max + p) * HD;
                kc[dst + 2 * i] = r0; kc[dst + 2 * i + 1] = r1;
                vc[dst + 2 * i] = vnew[2 * i]; vc[dst + 2 * i + 1] = vnew[2 * i + 1];
            }
        }
    }
    __syncthreads();
    // ---- attention: one wave per (batch row, q head)
    constexpr int LPR = HD / 8;                                              // lanes per value row (16)
    const int sub = lane % LPR, gq = lane / LPR;                             // 8-column slice, group within a quartet
    for (int hb = wave; hb < NB * H; hb += (int)(blockDim.x >> 6)) {
        const int b = hb / H, h = hb % H, kvh = h / rep;
        const int p = pos[b], n = p + 1;
        const float* q = qs + ((size_t)b * H + h) * HD;
        const float* knew = kn + ((size_t)b * KV + kvh) * HD;
        const bf16_t* Kc = kc + ((size_t)b * KV + kvh) * S_max * HD;
        const bf16_t* Vc = vc + ((size_t)b * KV + kvh) * S_max * HD;
        const bf16_t* vnew = qkv + (size_t)b * ldq + (H + KV + kvh) * HD;
        float d = 0.f;
        if (lane < n) {
            if (lane == p) {
#pragma unroll 8
                for (int c = 0; c < HD; ++c) d += q[c] * knew[c];
            } else {
                for (int c = 0; c < HD / 8; ++c) {
                    float kf[8];
                    unpack8(*reinterpret_cast<const U4*>(Kc + (size_t)lane * HD + c * 8), kf);
#pragma unroll
                    for (int j = 0; j < 8; ++j) d += q[c * 8 + j] * kf[j];
                }
            }
            d *= scale;
        }
        const float mx = wave_max(lane < n ? d : -INFINITY);
        const float pr = lane < n ? __expf(d - mx) : 0.f;
        const float sum = wave_sum(pr);
        pw[wave * 64 + lane] = pr;                                           // (wave-private: a wave's own LDS operations are in order)
        float o8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o8[j] = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                        // quartet r: key groups 4r .. 4r+3, mine is 4r + gq
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int s_ = 4 * r + gq; s_ < n; s_ += 16) {
                float vf[8];
                unpack8(*reinterpret_cast<const U4*>((s_ == p ? vnew : Vc + (size_t)s_ * HD) + sub * 8), vf);
                const float ps = pw[wave * 64 + s_];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += ps * vf[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[j] += lane_xor<LPR>(acc[j]);
                acc[j] += lane_xor<2 * LPR>(acc[j]);
                o8[j] += acc[j];                                             // quartets left to right, starting from 0 (0 + W0 is exact)
            }
        }
        if (gq == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xs[(size_t)b * K + h * HD + sub * 8 + j] = f2bf(o8[j] / sum);
        }
    }
    __syncthreads();
    // ---- y = attention . W^T (+ R): one wave per output row (gemv_kernel's loop)
    const int wpb = blockDim.x >> 6;
    for (int nrow = blockIdx.x * wpb + wave; nrow < N; nrow += gridDim.x * wpb) {
        float acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = 0.f;
        const bf16_t* w = W + (size_t)nrow * ldw;
        if (pre && nrow == row0) {                       // (wave-uniform) the prefetched row: the same chunks in the same order
#pragma unroll
            for (int c = 0; c < KCH; ++c) {
                const int k = lane * 8 + 512 * c;
                float wf[8];
                unpack8(wq0[c], wf);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float xf[8];
                    unpack8(*reinterpret_cast<const U4*>(xs + b * K + k), xf);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[b] += wf[j] * xf[j];
                }
            }
        } else {
            for (int k = lane * 8; k < K; k += 512) {
                float wf[8];
                unpack8(*reinterpret_cast<const U4*>(w + k), wf);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float xf[8];
                    unpack8(*reinterpret_cast<const U4*>(xs + b * K + k), xf);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[b] += wf[j] * xf[j];
                }
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float v = wave_sum(acc[b]);
            if (lane == 0) {
                if (R) v += bf2f(R[(size_t)b * ldy + nrow]);
                y[(size_t)b * ldy + nrow] = f2bf(v);
            }
        }
    }
}

// The same layer step for ONE utterance whose position the HOST knows (round 4): the depth decoder's step i is always at position
// i, so the captured frame graph can carry it as a kernel argument.  With the position in a register every address of the
// prologue - the RoPE table row, the q|k|v row, the <= 31 cached key rows, the value slices, the first weight row - is known when
// the wave starts, and all of them are requested at once: one memory round trip instead of the dependent chain of
// gemv_attn_kernel (position -> q|k|v row and table -> key rows -> value rows).  The cached key rows are fetched as contiguous
// 16-byte chunks (512 threads x 16 B = a kv head's 31 rows in one coalesced request each; `lane = key` loads touched 32 cache lines
// per instruction and took 1.9 us to issue, tools/probes/decode_stamps.py) and re-read from LDS in the lane = key layout (row
// stride 272 B: conflict-free); the rotated new key is written into the same LDS image, so that lane takes the same code path
// instead of a divergent serial dot product.  The arithmetic is gemv_attn_kernel<1, 128>'s operation for operation (same products,
// same order, same trees): bit-identical.  512 threads: wave w = q head w in the attention (H <= 8); S_max <= 32 (a frame's codebooks).
template <int HD>
__global__ __launch_bounds__(512) void gemv_attn_at_kernel(const bf16_t* __restrict__ qkv, bf16_t* kc, bf16_t* vc, int p,
                                                           const float* __restrict__ table, const bf16_t* __restrict__ W,
                                                           bf16_t* __restrict__ y, const bf16_t* __restrict__ R, int N, int H, int KV,
                                                           int S_max, int ldw, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    static_assert(HD == 128, "lane = column pair in the P.V phase");
    constexpr int KROW = HD * 2 + 16;                                       // bytes per key row of the LDS image (conflict-free lane = key reads)
    constexpr int VROW = HD * 2;                                            // value rows are read lane = column pair: no padding
    const int K = H * HD;
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem_x);                         // [K]
    float* qs = reinterpret_cast<float*>(smem_x + (size_t)K * 2);           // [H][HD]
    float* pw = qs + (size_t)H * HD;                                        // [8][32] probabilities (un-normalised), then [8] their sums
    float* psum = pw + 256;
    char* ks = reinterpret_cast<char*>(psum + 8);                           // [KV][32][KROW] key rows 0 .. p (row p: the new, rotated key)
    char* vs = ks + (size_t)KV * 32 * KROW;                                 // [KV][32][VROW] value rows 0 .. p
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rep = H / KV, n = p + 1;
    constexpr int KCH = 2;
    STAMP_DECL;
    STAMP(0);
    // ---- every load of the prologue, back to back, in the order they are consumed (loads return in order: the weight row, which
    //      comes from furthest away and is needed last, goes last)
    const int row0 = blockIdx.x * 8 + wave;
    const int npair = (H + KV) * (HD / 2);                                  // 640 pairs over 512 threads: two rounds
    float rc[2], rs[2], rx0[2], rx1[2];
    uint32_t rv[2] = {0u, 0u};                                              // (k-head pairs: the new value's pair beside it)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int it = threadIdx.x + 512 * t;
        rc[t] = rs[t] = rx0[t] = rx1[t] = 0.f;
        if (it < npair) {
            const int i = it % (HD / 2), hh = it / (HD / 2);
            const float2 cs = *reinterpret_cast<const float2*>(table + ((size_t)p * (HD / 2) + i) * 2);
            const uint32_t xx = *reinterpret_cast<const uint32_t*>(qkv + hh * HD + 2 * i);
            if (hh >= H) rv[t] = *reinterpret_cast<const uint32_t*>(qkv + (hh + KV) * HD + 2 * i);
            rc[t] = cs.x; rs[t] = cs.y; rx0[t] = __uint_as_float(xx << 16); rx1[t] = __uint_as_float(xx & 0xffff0000u);
        }
    }
    // cached key / value rows 0 .. p-1 of both kv heads: thread t = 16-byte chunk t of the head's contiguous rows (HD / 8 chunks per row)
    U4 kg[2] = {}, vg[2] = {};
    const bool kld = (int)threadIdx.x < p * (HD / 8);
    if (kld) {
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
            if (kh < KV) kg[kh] = *reinterpret_cast<const U4*>(kc + (size_t)kh * S_max * HD + (size_t)threadIdx.x * 8);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
            if (kh < KV) vg[kh] = *reinterpret_cast<const U4*>(vc + (size_t)kh * S_max * HD + (size_t)threadIdx.x * 8);
    }
    U4 wq0[KCH] = {};
    if (row0 < N) {
#pragma unroll
        for (int c = 0; c < KCH; ++c) wq0[c] = *reinterpret_cast<const U4*>(W + (size_t)row0 * ldw + lane * 8 + 512 * c);
    }
    STAMP(1);
#ifdef CSM_DECODE_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (probe: everything requested above has arrived)
    STAMP(2);
#endif
    // ---- RoPE of q and of the new k (-> row p of the key image; the new value -> row p of the value image); workgroup 0 appends
    //      k, v to the caches (row p: no load above reads it); then the cached rows into the images
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int it = threadIdx.x + 512 * t;
        if (it < npair) {
            const int i = it % (HD / 2), hh = it / (HD / 2);
            float y0 = rx0[t], y1 = rx1[t];
            rope_rot(y0, y1, rc[t], rs[t]);
            const bf16_t r0 = f2bf(y0), r1 = f2bf(y1);
            if (hh < H) {
                qs[(size_t)hh * HD + 2 * i] = bf2f(r0); qs[(size_t)hh * HD + 2 * i + 1] = bf2f(r1);
            } else {
                const int kh = hh - H;
                const uint32_t kk = (uint32_t)r0 | ((uint32_t)r1 << 16);
                *reinterpret_cast<uint32_t*>(ks + ((size_t)kh * 32 + p) * KROW + 4 * i) = kk;
                *reinterpret_cast<uint32_t*>(vs + ((size_t)kh * 32 + p) * VROW + 4 * i) = rv[t];
                if (blockIdx.x == 0) {
                    const size_t dst = ((size_t)kh * S_max + p) * HD + 2 * i;
                    *reinterpret_cast<uint32_t*>(kc + dst) = kk;
                    *reinterpret_cast<uint32_t*>(vc + dst) = rv[t];
                }
            }
        }
    }
    if (kld) {
        const int row = threadIdx.x / (HD / 8), ch = threadIdx.x % (HD / 8);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
            if (kh < KV) {
                *reinterpret_cast<U4*>(ks + ((size_t)kh * 32 + row) * KROW + ch * 16) = kg[kh];
                *reinterpret_cast<U4*>(vs + ((size_t)kh * 32 + row) * VROW + ch * 16) = vg[kh];
            }
    }
    lds_barrier();
    STAMP(3);
    // ---- scores + softmax: waves 0 .. H/2-1, two heads of one kv group per wave (lanes 0-31: head 2w, lanes 32-63: head 2w+1;
    //      lane & 31 = key).  attn_decode_kernel's arithmetic: a serial dot over HD per key; max and sum as 64-lane butterflies whose
    //      xor-32 step meets only -inf / 0 there (at most 32 keys) and is an identity - the xor-16 .. xor-1 steps stay inside a half.
    if (wave < H / 2) {
        const int hh = 2 * wave + (lane >> 5), key = lane & 31, kvh = hh / rep;
        const float* q = qs + (size_t)hh * HD;
        float d = 0.f;
        if (key < n) {
            const char* krow = ks + ((size_t)kvh * 32 + key) * KROW;
#pragma unroll
            for (int c = 0; c < HD / 8; ++c) {
                float kf[8];
                unpack8(*reinterpret_cast<const U4*>(krow + c * 16), kf);
#pragma unroll
                for (int j = 0; j < 8; ++j) d += q[c * 8 + j] * kf[j];
            }
            d *= scale;
        }
        float mx = key < n ? d : -INFINITY;
        mx = fmaxf(mx, lane_xor<16>(mx)); mx = fmaxf(mx, lane_xor<8>(mx)); mx = fmaxf(mx, lane_xor<4>(mx));
        mx = fmaxf(mx, lane_xor<2>(mx)); mx = fmaxf(mx, lane_xor<1>(mx));
        const float pr = key < n ? __expf(d - mx) : 0.f;
        float sum = pr;
        sum += lane_xor<16>(sum); sum += lane_xor<8>(sum); sum += lane_xor<4>(sum); sum += lane_xor<2>(sum); sum += lane_xor<1>(sum);
        pw[hh * 32 + key] = pr;
        if (key == 0) psum[hh] = sum;
    }
    STAMP(4);
    lds_barrier();
    // ---- P.V: wave = head, lane = column pair, no cross-lane traffic.  The reference order per column (attn_decode_kernel): 16 key
    //      groups (quartet r, group g: keys 4r + g and 4r + g + 16, accumulated from 0 by fused multiply-adds), a quartet's groups
    //      summed (g0 + g1) + (g2 + g3), the quartets added left to right starting from 0 - evaluated here by ONE lane per column
    //      pair instead of 4 x 16 lanes and two cross-lane sums per quartet: the same operations on the same operands.
    if (wave < H) {
        const int h = wave, kvh = h / rep;
        const float* ph = pw + h * 32;
        const char* vcol = vs + (size_t)kvh * 32 * VROW + lane * 4;
        float o0 = 0.f, o1 = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a0[4], a1[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                a0[g4] = 0.f; a1[g4] = 0.f;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int s_ = 4 * r + g4 + 16 * u;
                    if (s_ < n) {                                            // (uniform: n is a launch argument)
                        const uint32_t vv = *reinterpret_cast<const uint32_t*>(vcol + (size_t)s_ * VROW);
                        const float ps = ph[s_];
                        a0[g4] = __builtin_fmaf(ps, __uint_as_float(vv << 16), a0[g4]);
                        a1[g4] = __builtin_fmaf(ps, __uint_as_float(vv & 0xffff0000u), a1[g4]);
                    }
                }
            }
            o0 += (a0[0] + a0[1]) + (a0[2] + a0[3]);
            o1 += (a1[0] + a1[1]) + (a1[2] + a1[3]);
        }
        const float sum = psum[h];
        *reinterpret_cast<uint32_t*>(xs + h * HD + 2 * lane) = (uint32_t)f2bf(o0 / sum) | ((uint32_t)f2bf(o1 / sum) << 16);
    }
    lds_barrier();
    STAMP(5);
    // ---- y = attention . W^T (+ R): one wave per output row
    for (int nrow = row0; nrow < N; nrow += gridDim.x * 8) {
        float acc = 0.f;
        const bf16_t* w = W + (size_t)nrow * ldw;
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            const int k = lane * 8 + 512 * c;
            float wf[8], xf[8];
            unpack8(nrow == row0 ? wq0[c] : *reinterpret_cast<const U4*>(w + k), wf);
            unpack8(*reinterpret_cast<const U4*>(xs + k), xf);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += wf[j] * xf[j];
        }
        float v = wave_sum(acc);
        if (lane == 0) {
            if (R) v += bf2f(R[nrow]);
            y[nrow] = f2bf(v);
        }
    }
    STAMP(6);
    STAMP_FLUSH(200);
}

// The depth decoder's attention for two to four utterances (round 4; generate_batch), position known on the host: the scores and
// P.V phases of gemv_attn_at_kernel as a launch of their own - one workgroup per (batch row, kv head), its four q heads on four
// waves - where the fused form would make every workgroup of the output projection recompute all rows' attention (measured in
// round 3: slower from two rows on).  Same loads-at-once prologue, same coalesced key / value images, same arithmetic as
// attn_decode_kernel<128> operation for operation: bit-identical.  H = 4 KV, S_max <= 32.
template <int HD>
__global__ __launch_bounds__(256) void attn_decode_at_kernel(const bf16_t* __restrict__ qkv, bf16_t* kc, bf16_t* vc, bf16_t* __restrict__ out,
                                                             int p, const float* __restrict__ table, int H, int KV, int S_max, int ld,
                                                             float scale) {
    static_assert(HD == 128, "lane = column pair in the P.V phase");
    constexpr int KROW = HD * 2 + 16, VROW = HD * 2;
    __shared__ __attribute__((aligned(16))) float qs[4][HD];
    __shared__ float pw[4][32], psum[4];
    __shared__ __attribute__((aligned(16))) char ks[32 * KROW];
    __shared__ __attribute__((aligned(16))) char vs[32 * VROW];
    const int kvh = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = p + 1;
    const bf16_t* row = qkv + (size_t)b * ld;
    bf16_t* Kc = kc + ((size_t)b * KV + kvh) * S_max * HD;
    bf16_t* Vc = vc + ((size_t)b * KV + kvh) * S_max * HD;
    // ---- every load at once: RoPE inputs of the group's four q heads and its k head (5 x 64 pairs over 256 threads: two rounds),
    //      the new value beside the k pairs, the cached rows as contiguous 16-byte chunks (two per thread and image)
    float rc[2], rs[2], rx0[2], rx1[2];
    uint32_t rv[2] = {0u, 0u};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int it = threadIdx.x + 256 * t;
        rc[t] = rs[t] = rx0[t] = rx1[t] = 0.f;
        if (it < 5 * (HD / 2)) {
            const int i = it % (HD / 2), hh = it / (HD / 2);                 // hh < 4: q head 4 kvh + hh; hh == 4: the k head
            const float2 cs = *reinterpret_cast<const float2*>(table + ((size_t)p * (HD / 2) + i) * 2);
            const int col = (hh < 4 ? (4 * kvh + hh) : (H + kvh)) * HD + 2 * i;
            const uint32_t xx = *reinterpret_cast<const uint32_t*>(row + col);
            if (hh == 4) rv[t] = *reinterpret_cast<const uint32_t*>(row + (H + KV + kvh) * HD + 2 * i);
            rc[t] = cs.x; rs[t] = cs.y; rx0[t] = __uint_as_float(xx << 16); rx1[t] = __uint_as_float(xx & 0xffff0000u);
        }
    }
    U4 kg[2] = {}, vg[2] = {};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ch = threadIdx.x + 256 * t;
        if (ch < p * (HD / 8)) {
            kg[t] = *reinterpret_cast<const U4*>(Kc + (size_t)ch * 8);
            vg[t] = *reinterpret_cast<const U4*>(Vc + (size_t)ch * 8);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int it = threadIdx.x + 256 * t;
        if (it < 5 * (HD / 2)) {
            const int i = it % (HD / 2), hh = it / (HD / 2);
            float y0 = rx0[t], y1 = rx1[t];
            rope_rot(y0, y1, rc[t], rs[t]);
            const bf16_t r0 = f2bf(y0), r1 = f2bf(y1);
            if (hh < 4) {
                qs[hh][2 * i] = bf2f(r0); qs[hh][2 * i + 1] = bf2f(r1);
            } else {
                const uint32_t kk = (uint32_t)r0 | ((uint32_t)r1 << 16);
                *reinterpret_cast<uint32_t*>(ks + (size_t)p * KROW + 4 * i) = kk;
                *reinterpret_cast<uint32_t*>(vs + (size_t)p * VROW + 4 * i) = rv[t];
                *reinterpret_cast<uint32_t*>(Kc + (size_t)p * HD + 2 * i) = kk;        // (row p: no load above reads it)
                *reinterpret_cast<uint32_t*>(Vc + (size_t)p * HD + 2 * i) = rv[t];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ch = threadIdx.x + 256 * t;
        if (ch < p * (HD / 8)) {
            const int r_ = ch / (HD / 8), c_ = ch % (HD / 8);
            *reinterpret_cast<U4*>(ks + (size_t)r_ * KROW + c_ * 16) = kg[t];
            *reinterpret_cast<U4*>(vs + (size_t)r_ * VROW + c_ * 16) = vg[t];
        }
    }
    lds_barrier();
    // ---- scores + softmax: waves 0, 1 - two heads per wave in lane halves (see gemv_attn_at_kernel)
    if (wave < 2) {
        const int hh = 2 * wave + (lane >> 5), key = lane & 31;
        const float* q = qs[hh];
        float d = 0.f;
        if (key < n) {
            const char* krow = ks + (size_t)key * KROW;
#pragma unroll
            for (int c = 0; c < HD / 8; ++c) {
                float kf[8];
                unpack8(*reinterpret_cast<const U4*>(krow + c * 16), kf);
#pragma unroll
                for (int j = 0; j < 8; ++j) d += q[c * 8 + j] * kf[j];
            }
            d *= scale;
        }
        float mx = key < n ? d : -INFINITY;
        mx = fmaxf(mx, lane_xor<16>(mx)); mx = fmaxf(mx, lane_xor<8>(mx)); mx = fmaxf(mx, lane_xor<4>(mx));
        mx = fmaxf(mx, lane_xor<2>(mx)); mx = fmaxf(mx, lane_xor<1>(mx));
        const float pr = key < n ? __expf(d - mx) : 0.f;
        float sum = pr;
        sum += lane_xor<16>(sum); sum += lane_xor<8>(sum); sum += lane_xor<4>(sum); sum += lane_xor<2>(sum); sum += lane_xor<1>(sum);
        pw[hh][key] = pr;
        if (key == 0) psum[hh] = sum;
    }
    lds_barrier();
    // ---- P.V: wave = head of the group, lane = column pair, the reference's summation tree (see gemv_attn_at_kernel)
    {
        const float* ph = pw[wave];
        const char* vcol = vs + lane * 4;
        float o0 = 0.f, o1 = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a0[4], a1[4];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                a0[g4] = 0.f; a1[g4] = 0.f;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int s_ = 4 * r + g4 + 16 * u;
                    if (s_ < n) {
                        const uint32_t vv = *reinterpret_cast<const uint32_t*>(vcol + (size_t)s_ * VROW);
                        const float ps = ph[s_];
                        a0[g4] = __builtin_fmaf(ps, __uint_as_float(vv << 16), a0[g4]);
                        a1[g4] = __builtin_fmaf(ps, __uint_as_float(vv & 0xffff0000u), a1[g4]);
                    }
                }
            }
            o0 += (a0[0] + a0[1]) + (a0[2] + a0[3]);
            o1 += (a1[0] + a1[1]) + (a1[2] + a1[3]);
        }
        const float sum = psum[wave];
        *reinterpret_cast<uint32_t*>(out + (size_t)b * H * HD + (4 * kvh + wave) * HD + 2 * lane) =
            (uint32_t)f2bf(o0 / sum) | ((uint32_t)f2bf(o1 / sum) << 16);
    }
}

// The first half of a LoRA group's K-extension at decode time: t[b][0:kx] = s * x^[b] . At, rounded to bf16 once (the rounding of
// LoRAGroup.project in training), x^ = x or - norm_w != NULL - x RMS-normalised exactly as the gemv prologues leave it (sum of
// squares over lane-strided 8-element chunks of one wave, wave_sum, x * rstd * w rounded to bf16), so the adapters see the same
// input as the frozen product they extend.  At [K][lda] is read in its arena layout.  One workgroup per 8 columns of t; thread i
// takes rows k = i, i + 512, ... of At (16 bytes each) and every batch row; partials are reduced by wave butterflies and then
// across the eight waves in a fixed order: deterministic, and row b never depends on the other rows.
template <int NB>
__global__ __launch_bounds__(512) void lora_project_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ At, bf16_t* __restrict__ t,
                                                           int K, int ldx, int lda, int ldt, const bf16_t* __restrict__ norm_w, float eps,
                                                           float scale) {
    __shared__ float rs[4];
    __shared__ float part[8][NB][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 8;
    if (norm_w) {
        if (wave < NB) {
            float ss = 0.f;
            for (int c = lane; c < (K >> 3); c += 64) {
                float f[8];
                unpack8(*reinterpret_cast<const U4*>(x + (size_t)wave * ldx + c * 8), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
            }
            ss = wave_sum(ss);
            if (lane == 0) rs[wave] = rsqrtf(ss / (float)K + eps);
        }
        __syncthreads();
    }
    float r[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) r[b] = norm_w ? rs[b] : 1.f;
    float acc[NB][8];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[b][j] = 0.f;
#pragma unroll 4
    for (int k = threadIdx.x; k < K; k += 512) {
        float a[8];
        unpack8(*reinterpret_cast<const U4*>(At + (size_t)k * lda + c0), a);
        const float w = norm_w ? bf2f(norm_w[k]) : 1.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float xv = bf2f(x[(size_t)b * ldx + k]);
            if (norm_w) xv = bf2f(f2bf(xv * r[b] * w));
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[b][j] += xv * a[j];
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = wave_sum(acc[b][j]);
            if (lane == 0) part[wave][b][j] = v;
        }
    __syncthreads();
    if ((int)threadIdx.x < NB * 8) {
        const int b = threadIdx.x >> 3, j = threadIdx.x & 7;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += part[w][b][j];
        t[(size_t)b * ldt + c0 + j] = f2bf(scale * v);
    }
}

// lora_project_kernel with one adapter per batch row (csm_lora_project_rows_bf16): row b reads At[a_b] and scales by scale[a_b],
// a_b = row_adapter[b]; -1 (or out of range) writes exact zeros.  Rows go in groups of NB <= 4 per workgroup on the grid's second
// axis.  A row's operations and their order are lora_project_kernel's for that row (thread-strided k, wave_sum, the waves' partials
// in fixed order - none of which depends on NB or on the other rows), so each row is bit-identical to a one-row
// csm_lora_project_bf16 launch with its own At and scale.
template <int NB>
__global__ __launch_bounds__(512) void lora_project_rows_kernel(const bf16_t* __restrict__ x, const bf16_t* const* __restrict__ At_tab,
                                                                bf16_t* __restrict__ t, const int* __restrict__ row_adapter,
                                                                const float* __restrict__ scale_tab, int nad, int B, int K, int ldx,
                                                                int lda, int ldt, const bf16_t* __restrict__ norm_w, float eps) {
    __shared__ float rs[4];
    __shared__ float part[8][NB][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 8, b0 = blockIdx.y * NB;
    int ad[NB];
    const bf16_t* At[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int a = b0 + b < B ? row_adapter[b0 + b] : -1;
        ad[b] = a < nad ? a : -1;
        At[b] = ad[b] >= 0 ? At_tab[ad[b]] : nullptr;
    }
    if (norm_w) {
        if (wave < NB && ad[wave] >= 0) {
            float ss = 0.f;
            for (int c = lane; c < (K >> 3); c += 64) {
                float f[8];
                unpack8(*reinterpret_cast<const U4*>(x + (size_t)(b0 + wave) * ldx + c * 8), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
            }
            ss = wave_sum(ss);
            if (lane == 0) rs[wave] = rsqrtf(ss / (float)K + eps);
        }
        __syncthreads();
    }
    float r[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) r[b] = (norm_w && ad[b] >= 0) ? rs[b] : 1.f;
    float acc[NB][8];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[b][j] = 0.f;
#pragma unroll 4
    for (int k = threadIdx.x; k < K; k += 512) {
        const float w = norm_w ? bf2f(norm_w[k]) : 1.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (ad[b] < 0) continue;                             // (workgroup-uniform)
            float a[8];
            unpack8(*reinterpret_cast<const U4*>(At[b] + (size_t)k * lda + c0), a);
            float xv = bf2f(x[(size_t)(b0 + b) * ldx + k]);
            if (norm_w) xv = bf2f(f2bf(xv * r[b] * w));
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[b][j] += xv * a[j];
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = wave_sum(acc[b][j]);
            if (lane == 0) part[wave][b][j] = v;
        }
    __syncthreads();
    if ((int)threadIdx.x < NB * 8) {
        const int b = threadIdx.x >> 3, j = threadIdx.x & 7;
        if (b0 + b < B) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) v += part[w][b][j];
            t[(size_t)(b0 + b) * ldt + c0 + j] = ad[b] >= 0 ? f2bf(scale_tab[ad[b]] * v) : f2bf(0.f);
        }
    }
}

}  // namespace

#ifdef CSM_DECODE_STAMPS
// probe builds: copy out (and reset) the stamp records; returns the number of 10-word records
extern "C" int csm_decode_stamps(unsigned long long* host, int max_records) {
    unsigned int n = 0;
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_decode_nstamp), sizeof(n));
    int rec = (int)(n / 10); if (rec > max_records) rec = max_records; if (rec > 819) rec = 819;
    if (host && rec > 0) (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_decode_stamps), (size_t)rec * 10 * sizeof(unsigned long long));
    const unsigned int zero = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_decode_nstamp), &zero, sizeof(zero));
    return rec;
}
#endif
// (g_gemv_rpw: gate/up pairs per wave in the depth decoder's w13 product.  Measured at 1 / 2 / 4: 207.5 / 207.5 / 204 frames/s -
//  that launch streams 32 MB and is bound by its loads, not by the per-wave normalisation: one pair per wave stays the default)
// (g_gemv_mfma_small: B = 2..4 through gemv_mfma_kernel as well - A/B measurement only, off by default: it gives up the B <= 4
//  products' bit-equality with the one-row kernels)
// the decode product kernel the library launched last, with its template arguments (host bookkeeping only: the kernel-level tests
// assert with it which kernel took a case); written by the launchers below and by csm_gemv_fp8w (quant.hip)
// (a launcher only stores the arguments - a few host stores per launch; the name is put together when it is asked for)
CsmGemvLast g_last_gemv = {nullptr, "", {0, 0, 0, 0, 0, 0}};
extern "C" const char* csm_gemv_last_kernel(void) {
    static char name[128];
    const CsmGemvLast& l = g_last_gemv;
    name[0] = 0;
    if (l.fmt) (void)snprintf(name, sizeof(name), l.fmt, l.a[0], l.t, l.a[1], l.a[2], l.a[3], l.a[4], l.a[5]);
    return name;
}
// fmt takes (int, type name, int...) in this order: the first template argument, the output type, the rest
static inline void gemv_note(const char* fmt, int a0, const char* t, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0, int a5 = 0) {
    g_last_gemv.fmt = fmt; g_last_gemv.t = t;
    g_last_gemv.a[0] = a0; g_last_gemv.a[1] = a1; g_last_gemv.a[2] = a2; g_last_gemv.a[3] = a3; g_last_gemv.a[4] = a4; g_last_gemv.a[5] = a5;
}
static int g_gemv_reg = 1, g_gemv_nt = 1, g_gemv_rpw = 1, g_gemv_regn = 1, g_gemv_mfma_small = 0;   // csm_set_decode_tuning (A/B: tools/probes)
extern "C" int csm_set_decode_tuning(int key, int value) {
    if (key == 0) g_gemv_reg = value; else if (key == 1) g_gemv_nt = value; else if (key == 2) g_gemv_rpw = value;
    else if (key == 3) g_gemv_regn = value; else if (key == 4) g_gemv_mfma_small = value; else return 1;
    return 0;
}
// ext: empty (the plain products) or one GemvExt (csm_gemv_bf16_kext): the same dispatch, the kernels' trailing pack
template <typename... Ext>
static int gemv_launch(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw, int ldx, int ldy,
                       int out_f32, const void* norm_w, float eps, int swiglu, const int* row_index, int row_offset,
                       hipStream_t stream, Ext... ext) {
    CSM_REQUIRE(x && W && y && B >= 1 && B <= 16 && N > 0 && K > 0 && (K & 7) == 0 && (ldw & 7) == 0 && (ldx & 7) == 0,
                "csm_gemv_bf16: bad arguments (B=%d N=%d K=%d: needs 1 <= B <= 16)", B, N, K);
    CSM_REQUIRE(!swiglu || ((N & 1) == 0 && !out_f32), "csm_gemv_bf16_ex: the SwiGLU form needs an even N and bf16 output");
    if constexpr (ExtKind<Ext...>::v != 1) {             // (the plain products and the per-row extension dispatch alike)
        if (B > 4 || (B >= 2 && g_gemv_mfma_small && (K & 31) == 0)) {   // gemv_mfma.h
            const bool nt = g_gemv_nt && (K == 2048 || (K == 8192 && N == 2048));
            return gemv_mfma_launch<WeightBf16>({(const bf16_t*)W}, x, y, residual, B, N, K, ldw, ldx, ldy, out_f32, norm_w, eps, swiglu, row_index,
                                                row_offset, nt, stream, ext...);
        }
    } else {
        CSM_REQUIRE(B <= 4, "csm_gemv_bf16_kext: B=%d: the K-extension (live LoRA adapters) takes at most 4 batch rows", B);
    }
    CSM_REQUIRE((size_t)B * K * 2 <= 65536, "csm_gemv_bf16: B*K too large for the LDS copy of x");
    const int no = swiglu ? N / 2 : N;
    if (B == 1 && g_gemv_reg && (K == 1024 || K == 2048 || K == 8192)) {
        // one batch row: x in registers, no LDS, no barrier (gemv_reg_kernel); matrices of the 2048-wide stack are streamed once
        // per frame: non-temporal
        int grid = (no + 3) / 4;
        const bool nt = g_gemv_nt && (K == 2048 || (K == 8192 && N == 2048));
#define LR(KCH, T, SW, NT_) hipLaunchKernelGGL((gemv_reg_kernel<KCH, T, SW, NT_, 1, Ext...>), dim3(grid), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)W, (T*)y, (const bf16_t*)residual, N, ldw, ldx, ldy, (const bf16_t*)norm_w, eps, row_index, row_offset, ext...)
#define LK(T, SW, NT_) do { if (K == 1024) LR(2, T, SW, NT_); else if (K == 2048) LR(4, T, SW, NT_); else LR(16, T, SW, NT_); } while (0)
        if (swiglu && K == 1024 && !nt && g_gemv_rpw > 1 && no >= 2048) {
            // the depth decoder's w13: several gate/up pairs per wave (one normalisation of x per wave instead of per pair)
            if (g_gemv_rpw == 2) {
                grid = (no + 7) / 8;
                hipLaunchKernelGGL((gemv_reg_kernel<2, bf16_t, true, false, 2, Ext...>), dim3(grid), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)W, (bf16_t*)y, (const bf16_t*)residual, N, ldw, ldx, ldy, (const bf16_t*)norm_w, eps, row_index, row_offset, ext...);
            } else {
                grid = (no + 15) / 16;
                hipLaunchKernelGGL((gemv_reg_kernel<2, bf16_t, true, false, 4, Ext...>), dim3(grid), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)W, (bf16_t*)y, (const bf16_t*)residual, N, ldw, ldx, ldy, (const bf16_t*)norm_w, eps, row_index, row_offset, ext...);
            }
        }
        else if (swiglu) { if (nt) LK(bf16_t, true, true); else LK(bf16_t, true, false); }
        else if (out_f32) { if (nt) LK(float, false, true); else LK(float, false, false); }
        else { if (nt) LK(bf16_t, false, true); else LK(bf16_t, false, false); }
#undef LK
#undef LR
        {
            const bool rpw = swiglu && K == 1024 && !nt && g_gemv_rpw > 1 && no >= 2048;
            gemv_note("gemv_reg_kernel<%d, %s, %d, %d, %d, ext%d>", K / 512, (out_f32 && !swiglu) ? "float" : "bf16", swiglu ? 1 : 0,
                      nt ? 1 : 0, rpw ? (g_gemv_rpw == 2 ? 2 : 4) : 1, ExtKind<Ext...>::v);
        }
        CSM_CHECK_LAUNCH("csm_gemv_bf16");
        return 0;
    }
    if (B >= 2 && g_gemv_reg && g_gemv_regn && (K == 1024 || K == 2048 || (K == 8192 && !swiglu && !out_f32))) {
        // two to four batch rows, x in registers (gemv_regn_kernel)
        const int gridn = (no + 3) / 4;
        const bool nt = g_gemv_nt && (K == 2048 || (K == 8192 && N == 2048));
        const size_t ldsn = (size_t)B * K * sizeof(float);
#define LN(KCH, NB, T, SW, NT_, SC_) do { auto kf = gemv_regn_kernel<KCH, NB, T, SW, NT_, SC_, Ext...>;                                       \
            if (ldsn > 65536) { static bool done_ = false; if (!done_) { (void)hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsn); done_ = true; } } \
            hipLaunchKernelGGL(kf, dim3(gridn), dim3(256), ldsn, stream, (const bf16_t*)x, (const bf16_t*)W, (T*)y, (const bf16_t*)residual, N, ldw, ldx, ldy, (const bf16_t*)norm_w, eps, row_index, row_offset, ext...); } while (0)
#define LNB(KCH, T, SW, NT_, SC_) do { if (B == 2) LN(KCH, 2, T, SW, NT_, SC_); else if (B == 3) LN(KCH, 3, T, SW, NT_, SC_); else LN(KCH, 4, T, SW, NT_, SC_); } while (0)
#define LNK(T, SW) do { if (K == 1024) LNB(2, T, SW, false, 2); else if (nt) LNB(4, T, SW, true, 4); else LNB(4, T, SW, false, 4); } while (0)
        if (K == 8192) { if (nt) LNB(16, bf16_t, false, true, 4); else LNB(16, bf16_t, false, false, 4); }
        else if (swiglu) LNK(bf16_t, true); else if (out_f32) LNK(float, false); else LNK(bf16_t, false);
#undef LNK
#undef LNB
#undef LN
        gemv_note(B == 2 ? "gemv_regn_kernel<%d, 2, %s, %d, %d, %d, ext%d>" : B == 3 ? "gemv_regn_kernel<%d, 3, %s, %d, %d, %d, ext%d>"
                                                                                      : "gemv_regn_kernel<%d, 4, %s, %d, %d, %d, ext%d>",
                  K / 512, (out_f32 && !swiglu) ? "float" : "bf16", swiglu ? 1 : 0, (nt && K != 1024) ? 1 : 0, K == 1024 ? 2 : 4, ExtKind<Ext...>::v);
        CSM_CHECK_LAUNCH("csm_gemv_bf16");
        return 0;
    }
    const int grid = no / 4 < 1 ? 1 : (no / 4 > 2048 ? 2048 : no / 4);
    const size_t lds = (size_t)B * K * 2;
#define L(NB, T, SW) hipLaunchKernelGGL((gemv_kernel<NB, T, SW, Ext...>), dim3(grid), dim3(256), lds, stream, (const bf16_t*)x, (const bf16_t*)W, (T*)y, (const bf16_t*)residual, N, K, ldw, ldx, ldy, (const bf16_t*)norm_w, eps, row_index, row_offset, ext...)
    if (swiglu) { if (B == 1) L(1, bf16_t, true); else if (B == 2) L(2, bf16_t, true); else if (B == 3) L(3, bf16_t, true); else L(4, bf16_t, true); }
    else if (out_f32) { if (B == 1) L(1, float, false); else if (B == 2) L(2, float, false); else if (B == 3) L(3, float, false); else L(4, float, false); }
    else { if (B == 1) L(1, bf16_t, false); else if (B == 2) L(2, bf16_t, false); else if (B == 3) L(3, bf16_t, false); else L(4, bf16_t, false); }
#undef L
    gemv_note("gemv_kernel<%d, %s, %d, ext%d>", B, (out_f32 && !swiglu) ? "float" : "bf16", swiglu ? 1 : 0, ExtKind<Ext...>::v);
    CSM_CHECK_LAUNCH("csm_gemv_bf16");
    return 0;
}

extern "C" int csm_gemv_bf16(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw,
                             int ldx, int ldy, int out_f32, hipStream_t stream) {
    return gemv_launch(x, W, y, residual, B, N, K, ldw, ldx, ldy, out_f32, nullptr, 0.f, 0, nullptr, 0, stream);
}

extern "C" int csm_gemv_bf16_ex(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw,
                                int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu, const int* row_index,
                                int row_offset, hipStream_t stream) {
    return gemv_launch(x, W, y, residual, B, N, K, ldw, ldx, ldy, out_f32, norm_scale, eps, swiglu, row_index, row_offset, stream);
}

// csm_gemv_bf16_ex with a LoRA group's K-extension (GemvExt): y = epilogue(x^ W^T + ext_t ext_B^T + bias), ext_t from
// csm_lora_project_bf16.  Bit-identical to csm_gemv_bf16_ex when ext_B is all zeros.
extern "C" int csm_gemv_bf16_kext(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw,
                                  int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu, const int* row_index,
                                  int row_offset, const void* ext_t, const void* ext_B, int kx, int ld_ext_t, int ld_ext_B,
                                  const void* bias, hipStream_t stream) {
    CSM_REQUIRE(ext_t && ext_B && kx > 0 && kx <= 512 && (kx & 7) == 0 && ld_ext_t >= kx && ld_ext_B >= kx && (ld_ext_t & 7) == 0 &&
                (ld_ext_B & 7) == 0 && ((uintptr_t)ext_t & 15) == 0 && ((uintptr_t)ext_B & 15) == 0,
                "csm_gemv_bf16_kext: bad extension (kx=%d ld_t=%d ld_B=%d: needs kx <= 512, multiples of 8, 16-byte aligned rows)",
                kx, ld_ext_t, ld_ext_B);
    GemvExt e;
    e.t = (const bf16_t*)ext_t; e.Bx = (const bf16_t*)ext_B; e.bias = (const bf16_t*)bias;
    e.kx = kx; e.ldt = ld_ext_t; e.ldb = ld_ext_B;
    return gemv_launch(x, W, y, residual, B, N, K, ldw, ldx, ldy, out_f32, norm_scale, eps, swiglu, row_index, row_offset, stream, e);
}

// csm_gemv_bf16_kext with one adapter per batch row (GemvExtRows; a bank of adapters that share kx, ldb): B = 1..16.
extern "C" int csm_gemv_bf16_kext_rows(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw,
                                       int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu,
                                       const int* row_index, int row_offset, const void* ext_t, const void* const* ext_B,
                                       const void* const* bias, const int* row_adapter, int n_adapters, int kx, int ld_ext_t,
                                       int ld_ext_B, hipStream_t stream) {
    GemvExtRows e;
    if (const int rc = ext_rows_check("csm_gemv_bf16_kext_rows", e, B, ext_t, ext_B, bias, row_adapter, n_adapters, kx, ld_ext_t, ld_ext_B)) return rc;
    return gemv_launch(x, W, y, residual, B, N, K, ldw, ldx, ldy, out_f32, norm_scale, eps, swiglu, row_index, row_offset, stream, e);
}

extern "C" int csm_lora_project_rows_bf16(const void* x, const void* const* At, void* t, const int* row_adapter, const float* scale,
                                          int n_adapters, int B, int K, int kx, int ldx, int lda, int ldt, const void* norm_scale,
                                          float eps, hipStream_t stream) {
    CSM_REQUIRE(B >= 1 && B <= 16, "csm_lora_project_rows_bf16: B=%d: takes 1 to 16 batch rows", B);
    CSM_REQUIRE(x && At && t && row_adapter && scale && n_adapters >= 1 && K > 0 && (K & 7) == 0 && kx > 0 && (kx & 7) == 0 &&
                lda >= kx && ldt >= kx && (lda & 7) == 0 && (!norm_scale || ((ldx & 7) == 0 && ((uintptr_t)x & 15) == 0)),
                "csm_lora_project_rows_bf16: bad arguments (B=%d K=%d kx=%d lda=%d ldt=%d adapters=%d)", B, K, kx, lda, ldt, n_adapters);
    const int nb = B < 4 ? B : 4;
    const dim3 grid(kx / 8, (B + nb - 1) / nb);
#define L(NB) hipLaunchKernelGGL((lora_project_rows_kernel<NB>), grid, dim3(512), 0, stream, (const bf16_t*)x, (const bf16_t* const*)At, (bf16_t*)t, row_adapter, scale, n_adapters, B, K, ldx, lda, ldt, (const bf16_t*)norm_scale, eps)
    if (nb == 1) L(1); else if (nb == 2) L(2); else if (nb == 3) L(3); else L(4);
#undef L
    gemv_note("lora_project_rows_kernel<%d>%.0s", nb, "");
    CSM_CHECK_LAUNCH("csm_lora_project_rows_bf16");
    return 0;
}

extern "C" int csm_lora_project_bf16(const void* x, const void* At, void* t, int B, int K, int kx, int ldx, int lda, int ldt,
                                     float scale, const void* norm_scale, float eps, hipStream_t stream) {
    CSM_REQUIRE(x && At && t && B >= 1 && B <= 4 && K > 0 && (K & 7) == 0 && kx > 0 && (kx & 7) == 0 && lda >= kx && ldt >= kx &&
                (lda & 7) == 0 && ((uintptr_t)At & 15) == 0 && (!norm_scale || ((ldx & 7) == 0 && ((uintptr_t)x & 15) == 0)),
                "csm_lora_project_bf16: bad arguments (B=%d K=%d kx=%d lda=%d ldt=%d)", B, K, kx, lda, ldt);
#define L(NB) hipLaunchKernelGGL((lora_project_kernel<NB>), dim3(kx / 8), dim3(512), 0, stream, (const bf16_t*)x, (const bf16_t*)At, (bf16_t*)t, K, ldx, lda, ldt, (const bf16_t*)norm_scale, eps, scale)
    if (B == 1) L(1); else if (B == 2) L(2); else if (B == 3) L(3); else L(4);
#undef L
    gemv_note("lora_project_kernel<%d>%.0s", B, "");
    CSM_CHECK_LAUNCH("csm_lora_project_bf16");
    return 0;
}

extern "C" int csm_gemv_t_bf16(const void* x, const void* W, void* y, int B, int N, int K, int ldw, int ldx, int ldy,
                               int out_f32, hipStream_t stream) {
    CSM_REQUIRE(x && W && y && B >= 1 && B <= 4 && N > 0 && K > 0 && (ldw & 7) == 0, "csm_gemv_t_bf16: bad arguments");
    const int grid = ((N + 7) / 8 + 255) / 256;
#define L(NB, T) hipLaunchKernelGGL((gemv_t_kernel<NB, T>), dim3(grid), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)W, (T*)y, N, K, ldw, ldx, ldy)
    if (out_f32) { if (B == 1) L(1, float); else if (B == 2) L(2, float); else if (B == 3) L(3, float); else L(4, float); }
    else { if (B == 1) L(1, bf16_t); else if (B == 2) L(2, bf16_t); else if (B == 3) L(3, bf16_t); else L(4, bf16_t); }
#undef L
    gemv_note("gemv_t_kernel<%d, %s>", B, out_f32 ? "float" : "bf16");
    CSM_CHECK_LAUNCH("csm_gemv_t_bf16");
    return 0;
}

extern "C" int csm_kv_append(const void* qkv, void* kcache, void* vcache, const int* pos, int B, int H, int KV, int HD,
                             int S_max, int ld, hipStream_t stream) {
    CSM_REQUIRE(qkv && kcache && vcache && pos && B > 0 && H > 0 && KV > 0 && H % KV == 0 && (ld & 7) == 0, "csm_kv_append: bad arguments");
    CSM_REQUIRE(HD == 64 || HD == 128, "csm_kv_append: head_dim %d unsupported", HD);            // (the shapes csm_attn_decode reads back)
    CSM_REQUIRE(S_max >= 1 && S_max <= 8192, "csm_kv_append: S_max %d outside 1 .. 8192", S_max);
    hipLaunchKernelGGL(kv_append_kernel, dim3(B), dim3(256), 0, stream, (const bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache, pos, H,
                       KV, HD, S_max, ld);
    CSM_CHECK_LAUNCH("csm_kv_append");
    return 0;
}

extern "C" int csm_kv_shift(const void* src, void* dst, const float* rope_table, int table_rows, int layers, int KV, int HD, int len,
                            int keep, int drop, hipStream_t stream) {
    CSM_REQUIRE(src && dst && rope_table, "csm_kv_shift: null pointer");
    CSM_REQUIRE(HD == 64 || HD == 128, "csm_kv_shift: head_dim %d unsupported", HD);
    CSM_REQUIRE(layers >= 1 && KV >= 1 && (long long)layers * 2 * KV <= 0x7fffffffLL, "csm_kv_shift: %d layers x %d kv heads", layers, KV);
    CSM_REQUIRE(drop >= 1 && keep >= 0 && (long long)keep + drop <= len && len - drop >= 1,
                "csm_kv_shift: keep %d + drop %d of %d positions (needs drop >= 1, keep >= 0, keep + drop <= len, len - drop >= 1)", keep,
                drop, len);
    CSM_REQUIRE(drop < table_rows, "csm_kv_shift: drop %d outside the RoPE table (%d rows)", drop, table_rows);
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    CSM_REQUIRE((s0 & 15) == 0 && (d0 & 15) == 0, "csm_kv_shift: src and dst must be 16-byte aligned");
    const int planes = layers * 2 * KV, nl = len - drop;
    const size_t sbytes = (size_t)planes * len * HD * sizeof(bf16_t), dbytes = (size_t)planes * nl * HD * sizeof(bf16_t);
    CSM_REQUIRE(s0 + sbytes <= d0 || d0 + dbytes <= s0, "csm_kv_shift: dst overlaps src (the shift is out of place)");
    const float* trow = rope_table + (size_t)drop * HD;             // row `drop`: HD / 2 (cos, sin) pairs
    const dim3 grid((unsigned)(((long long)nl * (HD / 8) + 255) / 256), (unsigned)(planes < 65535 ? planes : 65535));
    if (HD == 64)
        hipLaunchKernelGGL((kv_shift_kernel<64>), grid, dim3(256), 0, stream, (const bf16_t*)src, (bf16_t*)dst, trow, planes, KV, len, keep, drop);
    else
        hipLaunchKernelGGL((kv_shift_kernel<128>), grid, dim3(256), 0, stream, (const bf16_t*)src, (bf16_t*)dst, trow, planes, KV, len, keep, drop);
    CSM_CHECK_LAUNCH("csm_kv_shift");
    return 0;
}

extern "C" int csm_kv_fork_rows(const void* const* src, void* kv, int* pos, const int* rows, const int* len, int R, int layers, int B,
                                 int KV, int HD, int S_max, hipStream_t stream) {
    CSM_REQUIRE(src && kv && pos && rows && len, "csm_kv_fork_rows: null pointer");
    CSM_REQUIRE(R >= 1 && R <= 16, "csm_kv_fork_rows: %d segments (1 to 16)", R);
    CSM_REQUIRE(HD == 64 || HD == 128, "csm_kv_fork_rows: head_dim %d unsupported", HD);
    CSM_REQUIRE(layers >= 1 && B >= 1 && KV >= 1 && S_max >= 1 && S_max <= (1 << 24) && (long long)layers * 2 * KV <= 0x7fffffffLL,
                "csm_kv_fork_rows: bad shape layers=%d B=%d KV=%d S_max=%d", layers, B, KV, S_max);
    const uintptr_t d0 = (uintptr_t)kv;
    const size_t dbytes = (size_t)layers * 2 * B * KV * S_max * HD * sizeof(bf16_t);
    CSM_REQUIRE((d0 & 15) == 0, "csm_kv_fork_rows: the cache must be 16-byte aligned");
    const int planes = layers * 2 * KV;
    ForkRows a = {};
    unsigned chunks = 0;
    for (int r = 0; r < R; ++r) {
        CSM_REQUIRE(src[r], "csm_kv_fork_rows: segment %d: null pointer", r);
        CSM_REQUIRE(len[r] >= 1 && len[r] <= S_max, "csm_kv_fork_rows: segment %d: %d positions outside 1 .. S_max = %d", r, len[r], S_max);
        CSM_REQUIRE(rows[r] >= 0 && rows[r] < B, "csm_kv_fork_rows: segment %d: batch row %d outside the caches (%d rows)", r, rows[r], B);
        for (int q = 0; q < r; ++q)
            CSM_REQUIRE(rows[q] != rows[r], "csm_kv_fork_rows: batch row %d appears in two segments (%d and %d)", rows[r], q, r);
        const uintptr_t s0 = (uintptr_t)src[r];
        CSM_REQUIRE((s0 & 15) == 0, "csm_kv_fork_rows: segment %d: the source must be 16-byte aligned", r);
        const size_t sbytes = (size_t)planes * len[r] * HD * sizeof(bf16_t);
        CSM_REQUIRE(s0 + sbytes <= d0 || d0 + dbytes <= s0, "csm_kv_fork_rows: segment %d: the source overlaps the cache", r);
        a.src[r] = (const bf16_t*)src[r]; a.row[r] = rows[r]; a.len[r] = len[r];
        chunks += (unsigned)((len[r] * (HD / 8) + 255) / 256);
    }
    const dim3 grid(chunks, (unsigned)((planes + 3) / 4 < 65535 ? (planes + 3) / 4 : 65535));
    if (HD == 64)
        hipLaunchKernelGGL((kv_fork_rows_kernel<64>), grid, dim3(256), 0, stream, a, (bf16_t*)kv, pos, planes, B, KV, S_max);
    else
        hipLaunchKernelGGL((kv_fork_rows_kernel<128>), grid, dim3(256), 0, stream, a, (bf16_t*)kv, pos, planes, B, KV, S_max);
    CSM_CHECK_LAUNCH("csm_kv_fork_rows");
    return 0;
}

extern "C" int csm_kv_park_rows(void* const* dst, const void* kv, const int* rows, const int* len, int R, int layers, int B, int KV,
                                 int HD, int S_max, hipStream_t stream) {
    CSM_REQUIRE(dst && kv && rows && len, "csm_kv_park_rows: null pointer");
    CSM_REQUIRE(R >= 1 && R <= 16, "csm_kv_park_rows: %d segments (1 to 16)", R);
    CSM_REQUIRE(HD == 64 || HD == 128, "csm_kv_park_rows: head_dim %d unsupported", HD);
    CSM_REQUIRE(layers >= 1 && B >= 1 && KV >= 1 && S_max >= 1 && S_max <= (1 << 24) && (long long)layers * 2 * KV <= 0x7fffffffLL,
                "csm_kv_park_rows: bad shape layers=%d B=%d KV=%d S_max=%d", layers, B, KV, S_max);
    const uintptr_t s0 = (uintptr_t)kv;
    const size_t sbytes = (size_t)layers * 2 * B * KV * S_max * HD * sizeof(bf16_t);
    CSM_REQUIRE((s0 & 15) == 0, "csm_kv_park_rows: the cache must be 16-byte aligned");
    const int planes = layers * 2 * KV;
    ParkRows a = {};
    unsigned chunks = 0;
    for (int r = 0; r < R; ++r) {
        CSM_REQUIRE(dst[r], "csm_kv_park_rows: segment %d: null pointer", r);
        CSM_REQUIRE(len[r] >= 1 && len[r] <= S_max, "csm_kv_park_rows: segment %d: %d positions outside 1 .. S_max = %d", r, len[r], S_max);
        CSM_REQUIRE(rows[r] >= 0 && rows[r] < B, "csm_kv_park_rows: segment %d: batch row %d outside the caches (%d rows)", r, rows[r], B);
        for (int q = 0; q < r; ++q)
            CSM_REQUIRE(rows[q] != rows[r], "csm_kv_park_rows: batch row %d appears in two segments (%d and %d)", rows[r], q, r);
        const uintptr_t d0 = (uintptr_t)dst[r];
        CSM_REQUIRE((d0 & 15) == 0, "csm_kv_park_rows: segment %d: the destination must be 16-byte aligned", r);
        const size_t dbytes = (size_t)planes * len[r] * HD * sizeof(bf16_t);
        CSM_REQUIRE(d0 + dbytes <= s0 || s0 + sbytes <= d0, "csm_kv_park_rows: segment %d: the destination overlaps the cache", r);
        for (int q = 0; q < r; ++q) {
            const uintptr_t q0 = (uintptr_t)dst[q];
            const size_t qbytes = (size_t)planes * len[q] * HD * sizeof(bf16_t);
            CSM_REQUIRE(d0 + dbytes <= q0 || q0 + qbytes <= d0, "csm_kv_park_rows: the destinations of segments %d and %d overlap", q, r);
        }
        a.dst[r] = (bf16_t*)dst[r]; a.row[r] = rows[r]; a.len[r] = len[r];
        chunks += (unsigned)((len[r] * (HD / 8) + 255) / 256);
    }
    const dim3 grid(chunks, (unsigned)((planes + 3) / 4 < 65535 ? (planes + 3) / 4 : 65535));
    if (HD == 64)
        hipLaunchKernelGGL((kv_park_rows_kernel<64>), grid, dim3(256), 0, stream, a, (const bf16_t*)kv, planes, B, KV, S_max);
    else
        hipLaunchKernelGGL((kv_park_rows_kernel<128>), grid, dim3(256), 0, stream, a, (const bf16_t*)kv, planes, B, KV, S_max);
    CSM_CHECK_LAUNCH("csm_kv_park_rows");
    return 0;
}

extern "C" int csm_sample_hist_move_rows(int* code_hist, int* hist_frame, int* packed, const int* rows, int R, int B, int K, int to_state,
                                          hipStream_t stream) {
    CSM_REQUIRE(code_hist && hist_frame && packed && rows, "csm_sample_hist_move_rows: null pointer");
    CSM_REQUIRE(R >= 1 && R <= 16, "csm_sample_hist_move_rows: %d rows (1 to 16)", R);
    CSM_REQUIRE(B >= 1 && K >= 1 && K <= 4096, "csm_sample_hist_move_rows: bad shape B=%d K=%d", B, K);
    CSM_REQUIRE(to_state == 0 || to_state == 1, "csm_sample_hist_move_rows: direction %d (0: to the packed buffer, 1: to the state)", to_state);
    const size_t n = (size_t)K * SMP_HIST;
    const uintptr_t p0 = (uintptr_t)packed, h0 = (uintptr_t)code_hist, f0 = (uintptr_t)hist_frame;
    const size_t pbytes = (size_t)R * (n + 1) * sizeof(int), hbytes = (size_t)B * n * sizeof(int), fbytes = (size_t)B * sizeof(int);
    CSM_REQUIRE(((p0 | h0 | f0) & 3) == 0, "csm_sample_hist_move_rows: the buffers must be 4-byte aligned");
    CSM_REQUIRE((p0 + pbytes <= h0 || h0 + hbytes <= p0) && (p0 + pbytes <= f0 || f0 + fbytes <= p0),
                "csm_sample_hist_move_rows: the packed buffer overlaps the state's rings or counters");
    HistRows a = {};
    for (int r = 0; r < R; ++r) {
        CSM_REQUIRE(rows[r] >= 0 && rows[r] < B, "csm_sample_hist_move_rows: entry %d: batch row %d outside the state (%d rows)", r, rows[r], B);
        for (int q = 0; q < r; ++q)
            CSM_REQUIRE(rows[q] != rows[r], "csm_sample_hist_move_rows: batch row %d appears in two entries (%d and %d)", rows[r], q, r);
        a.row[r] = rows[r];
    }
    hipLaunchKernelGGL(sample_hist_move_rows_kernel, dim3(R), dim3(256), 0, stream, a, code_hist, hist_frame, packed, K, to_state);
    CSM_CHECK_LAUNCH("csm_sample_hist_move_rows");
    return 0;
}

static int attn_decode_launch(const void* qkv, void* kcache, void* vcache, void* out, const int* pos, const float* table, int B,
                              int H, int KV, int HD, int S_max, int ld, hipStream_t stream) {
    CSM_REQUIRE(qkv && kcache && vcache && out && pos && B > 0 && H > 0 && KV > 0 && H % KV == 0 && (ld & 7) == 0, "csm_attn_decode: bad arguments");
    CSM_REQUIRE(HD == 64 || HD == 128, "csm_attn_decode: head_dim %d unsupported", HD);
    CSM_REQUIRE(S_max >= 1 && S_max <= 8192, "csm_attn_decode: S_max %d outside 1 .. 8192", S_max);
    const size_t lds = (size_t)(S_max + 16 + 6 * HD) * sizeof(float);
    const float scale = 1.f / sqrtf((float)HD);
    if (HD == 64)
        hipLaunchKernelGGL((attn_decode_kernel<64>), dim3(H, B), dim3(256), lds, stream, (const bf16_t*)qkv, (bf16_t*)kcache,
                           (bf16_t*)vcache, (bf16_t*)out, pos, H, KV, S_max, ld, scale, table);
    else
        hipLaunchKernelGGL((attn_decode_kernel<128>), dim3(H, B), dim3(256), lds, stream, (const bf16_t*)qkv, (bf16_t*)kcache,
                           (bf16_t*)vcache, (bf16_t*)out, pos, H, KV, S_max, ld, scale, table);
    CSM_CHECK_LAUNCH("csm_attn_decode");
    return 0;
}

extern "C" int csm_attn_decode(const void* qkv, const void* kcache, const void* vcache, void* out, const int* pos, int B, int H,
                               int KV, int HD, int S_max, int ld, hipStream_t stream) {
    return attn_decode_launch(qkv, const_cast<void*>(kcache), const_cast<void*>(vcache), out, pos, nullptr, B, H, KV, HD, S_max, ld,
                              stream);
}

extern "C" int csm_attn_decode_rope_at(const void* qkv, void* kcache, void* vcache, void* out, int pos, const float* rope_table,
                                       int B, int H, int KV, int HD, int S_max, int ld, hipStream_t stream) {
    CSM_REQUIRE(qkv && kcache && vcache && out && rope_table && B > 0, "csm_attn_decode_rope_at: bad arguments");
    CSM_REQUIRE(HD == 128 && H == 4 * KV && S_max >= 1 && S_max <= 32 && (ld & 7) == 0,
                "csm_attn_decode_rope_at: unsupported shape (H=%d KV=%d HD=%d S_max=%d: needs HD 128, H = 4 KV, S_max <= 32)", H, KV, HD, S_max);
    CSM_REQUIRE(pos >= 0 && pos < S_max, "csm_attn_decode_rope_at: position %d outside the cache (%d rows)", pos, S_max);
    hipLaunchKernelGGL((attn_decode_at_kernel<128>), dim3(KV, B), dim3(256), 0, stream, (const bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache,
                       (bf16_t*)out, pos, rope_table, H, KV, S_max, ld, 1.f / sqrtf((float)HD));
    CSM_CHECK_LAUNCH("csm_attn_decode_rope_at");
    return 0;
}

extern "C" int csm_attn_decode_rope(const void* qkv, void* kcache, void* vcache, void* out, const int* pos, const float* rope_table,
                                    int B, int H, int KV, int HD, int S_max, int ld, hipStream_t stream) {
    CSM_REQUIRE(rope_table, "csm_attn_decode_rope: null table");
    return attn_decode_launch(qkv, kcache, vcache, out, pos, rope_table, B, H, KV, HD, S_max, ld, stream);
}

// Decoder layer: rotate + cache append + attention over <= 64 cached positions + output projection (+ residual) in ONE launch;
// bit-identical to csm_attn_decode_rope followed by csm_gemv_bf16 (same arithmetic, see gemv_attn_kernel).  HD = 128 only.
extern "C" int csm_gemv_attn_at_bf16(const void* qkv, void* kcache, void* vcache, int pos, const float* rope_table, const void* W,
                                     void* y, const void* residual, int N, int H, int KV, int HD, int S_max, int ldw, hipStream_t stream) {
    CSM_REQUIRE(qkv && kcache && vcache && rope_table && W && y, "csm_gemv_attn_at_bf16: null pointer");
    CSM_REQUIRE(N > 0 && H > 0 && H <= 8 && (H & 1) == 0 && KV > 0 && KV <= 2 && H % KV == 0 && ((H / KV) & 1) == 0 && HD == 128 && H * HD == 1024 && S_max >= 1 && S_max <= 32 && (ldw & 7) == 0,
                "csm_gemv_attn_at_bf16: unsupported shape (H=%d KV=%d HD=%d S_max=%d: needs H*HD = 1024, HD 128, S_max <= 32)", H, KV, HD, S_max);
    CSM_REQUIRE(pos >= 0 && pos < S_max, "csm_gemv_attn_at_bf16: position %d outside the cache (%d rows)", pos, S_max);
    const int K = H * HD;
    const size_t lds = (size_t)K * 2 + ((size_t)H * HD + 256 + 8) * sizeof(float) + (size_t)KV * 32 * (HD * 2 + 16) + (size_t)KV * 32 * HD * 2;
    const int grid = N / 8 < 1 ? 1 : (N / 8 > 2048 ? 2048 : N / 8);
    const float scale = 1.f / sqrtf((float)HD);
    hipLaunchKernelGGL((gemv_attn_at_kernel<128>), dim3(grid), dim3(512), lds, stream, (const bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache,
                       pos, rope_table, (const bf16_t*)W, (bf16_t*)y, (const bf16_t*)residual, N, H, KV, S_max, ldw, scale);
    CSM_CHECK_LAUNCH("csm_gemv_attn_at_bf16");
    return 0;
}

extern "C" int csm_gemv_attn_bf16(const void* qkv, void* kcache, void* vcache, const int* pos, const float* rope_table, const void* W,
                                  void* y, const void* residual, int B, int N, int H, int KV, int HD, int S_max, int ld_qkv, int ldw,
                                  int ldy, hipStream_t stream) {
    CSM_REQUIRE(qkv && kcache && vcache && pos && rope_table && W && y, "csm_gemv_attn_bf16: null pointer");
    CSM_REQUIRE(B >= 1 && B <= 4 && N > 0 && H > 0 && KV > 0 && H % KV == 0 && HD == 128 && S_max >= 1 && S_max <= 64 && (ldw & 7) == 0 && (ld_qkv & 7) == 0,
                "csm_gemv_attn_bf16: unsupported shape (B=%d H=%d KV=%d HD=%d S_max=%d: needs HD 128, S_max <= 64)", B, H, KV, HD, S_max);
    const int K = H * HD;
    const size_t lds = (size_t)B * K * 2 + ((size_t)B * H * HD + (size_t)B * KV * HD + 512) * sizeof(float);
    CSM_REQUIRE(lds <= 65536, "csm_gemv_attn_bf16: %zu bytes of LDS needed", lds);
    const int grid = N / 8 < 1 ? 1 : (N / 8 > 2048 ? 2048 : N / 8);      // 8 waves per workgroup: one (row, head) each in the prologue
    const float scale = 1.f / sqrtf((float)HD);
#define L(NB) hipLaunchKernelGGL((gemv_attn_kernel<NB, 128>), dim3(grid), dim3(512), lds, stream, (const bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache, pos, rope_table, (const bf16_t*)W, (bf16_t*)y, (const bf16_t*)residual, N, H, KV, S_max, ld_qkv, ldw, ldy, scale)
    if (B == 1) L(1); else if (B == 2) L(2); else if (B == 3) L(3); else L(4);
#undef L
    CSM_CHECK_LAUNCH("csm_gemv_attn_bf16");
    return 0;
}
