// Band-limited sample-rate conversion on the device: the polyphase windowed-sinc interpolation of csm.data.resample
// (torchaudio's sinc_interp_hann) as a one-shot kernel and as a stateful streaming one for up to 16 streams a launch.
//
// For rates sr_in -> sr_out, g = gcd, o = sr_in / g, n = sr_out / g, T = 2 * width + o and a host-built table taps[n][T]:
//     y[j] = sum_{t = 0 .. T-1} taps[j mod n][t] * xbar[(j div n) * o - width + t],   xbar = x inside [0, N), 0 outside.
// Output block q = j div n is n outputs over the SAME T input samples, so the unit of work is a block: a workgroup takes a tile
// of QB consecutive blocks of one row, stages their input span ((QB - 1) * o + T samples, zeros where xbar is zero) and - when it
// fits - the whole table in LDS once, and every thread then owns whole outputs: one chain of T fmaf in ascending t, nothing
// shared, no atomics.  Both kernels go through resample_tile, so an output has the same bits whichever form computed it.
// The table rows are padded to an odd stride in LDS (lanes of a wave read n different rows at the same t: an even T would put
// them 2- or 4-way on one bank); the span reads are a broadcast or neighbours.  A table that does not fit LDS next to a span
// (more than RS_TAB_LDS floats) is read from global memory through the caches.
#include "common.h"
#include "csm_hip.h"

namespace {

constexpr int RS_LDS_FLOATS = 16384;     // 64 KB of LDS per workgroup: span + table
constexpr int RS_TAB_LDS = 14336;        // a padded table of up to 56 KB is staged; the span keeps at least 8 KB
constexpr int RS_MAX_T = 2048;           // taps per phase (a one-block span must fit the 8 KB)
constexpr long long RS_MAX_TABLE = 1LL << 22;    // table entries n * T (16 MB) - the limit on a rate pair
constexpr int RS_THREADS = 256;
constexpr int RS_TILE_OUT = 1024;        // outputs a workgroup aims for (4 per thread)

struct ResampleGeom {
    int o, n, width, T, Ts;   // Ts: row stride of the LDS table (odd)
    int QB;                   // output blocks per workgroup
    int span;                 // staged input samples per workgroup: (QB - 1) * o + T
    int tab_lds;              // the table is staged in LDS
};

// Outputs [blockIdx.x * QB * n, ...) of one row, counted from the row's first block of this launch.  fetch(i) is the input
// sample i of the row's window, whose sample 0 is the first sample of that first block (zeros where xbar is zero).  m outputs
// exist in the row.  Every thread of the workgroup must call (two barriers).
template <bool TAB_LDS, class Fetch>
__device__ __forceinline__ void resample_tile(const float* __restrict__ taps, const ResampleGeom g, int m, Fetch fetch,
                                              float* __restrict__ y) {
    extern __shared__ float rs_lds[];
    float* xs = rs_lds;                  // [span]
    float* tl = rs_lds + g.span;         // [n][Ts]
    const int b0 = blockIdx.x * g.QB;    // first block of the tile
    const int j0 = b0 * g.n;
    if (j0 >= m) return;                 // (uniform over the workgroup)
    int j1 = j0 + g.QB * g.n;
    if (j1 > m) j1 = m;
    const int blocks = (j1 - j0 + g.n - 1) / g.n;
    const int need = (blocks - 1) * g.o + g.T;
    for (int i = threadIdx.x; i < need; i += blockDim.x) xs[i] = fetch(b0 * g.o + i);
    if (TAB_LDS) {
        for (int p = threadIdx.x >> 6; p < g.n; p += blockDim.x >> 6)              // a wave per phase: coalesced rows
            for (int t = threadIdx.x & 63; t < g.T; t += 64) tl[p * g.Ts + t] = taps[(size_t)p * g.T + t];
    }
    __syncthreads();
    for (int j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
        const int ql = (j - j0) / g.n, p = (j - j0) - ql * g.n;
        const float* tp = TAB_LDS ? tl + p * g.Ts : taps + (size_t)p * g.T;
        const float* xp = xs + ql * g.o;
        float acc = 0.f;
        for (int t = 0; t < g.T; ++t) acc = fmaf(tp[t], xp[t], acc);              // THE order: ascending t, one fused chain
        y[j] = acc;
    }
}

// one-shot: x [R][N] -> y [R][M]; grid (tiles, R)
template <bool TAB_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                              float* __restrict__ y, ResampleGeom g, int N, int M) {
    const float* xr = x + (size_t)blockIdx.y * N;
    resample_tile<TAB_LDS>(taps, g, M, [&](int i) {
        const int s = i - g.width;                                   // block 0 starts width samples before the signal
        return s >= 0 && s < N ? xr[s] : 0.f;
    }, y + (size_t)blockIdx.y * M);
}

// The streams of one launch.  A row's window is [carry (H = T - 1 samples) | x (n_in new samples) | zeros]: the carry holds the
// last H samples before this call (zeros before the start of the stream), which reach back to the first sample of the first
// block not emitted yet - that block starts `off` samples into the window.
struct ResampleRows {
    const float* x[16];   // device pointers, one per row (may be NULL when n_in == 0)
    int slot[16];
    int par[16];
    int n_in[16];
    int off[16];          // window index of the first sample of the row's first new block
    int m[16];            // outputs the row emits in this call
};

// grid (tiles, R): carry arena [n_slots][2][H], y [R][ldy].  Tile 0 of every row also writes the row's next carry - the last H
// samples of [carry | x] - to the slot's other buffer, which nobody reads in this launch.
template <bool TAB_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_stream_rows_kernel(float* __restrict__ arena, const float* __restrict__ taps,
                                                                          float* __restrict__ y, ResampleRows rows, ResampleGeom g,
                                                                          long long ldy) {
    const int r = blockIdx.y;
    const int H = g.T - 1, n_in = rows.n_in[r];
    const float* carry = arena + ((size_t)rows.slot[r] * 2 + rows.par[r]) * H;
    const float* xr = rows.x[r];
    if (blockIdx.x == 0) {
        float* next = arena + ((size_t)rows.slot[r] * 2 + (rows.par[r] ^ 1)) * H;
        for (int i = threadIdx.x; i < H; i += blockDim.x) {
            const int v = n_in + i;
            next[i] = v < H ? carry[v] : xr[v - H];
        }
    }
    const int off = rows.off[r];
    resample_tile<TAB_LDS>(taps, g, rows.m[r], [&](int i) {
        const int v = off + i;
        return v < H ? carry[v] : (v - H < n_in ? xr[v - H] : 0.f);  // past the new samples: the zeros behind a stream's end
    }, y + (size_t)r * ldy);
}

// Checks a rate pair (reduced: o / n = sr_in / sr_out in lowest terms) and sizes the launch.
const char* resample_geom(ResampleGeom& g, int o, int n, int width) {
    if (o < 1 || n < 1 || width < 1) return "o, n and width must be >= 1";
    if (o == n) return "equal rates (o == n): nothing to resample";
    int a = o, b = n;
    while (b) { const int t = a % b; a = b; b = t; }
    if (a != 1) return "o / n is not in lowest terms";
    const long long T = 2LL * width + o;
    if (T > RS_MAX_T) return "more than 2048 taps per phase (T = 2 * width + o)";
    if ((long long)n * T > RS_MAX_TABLE) return "a table of more than 4 Mi entries (n * T)";
    g.o = o; g.n = n; g.width = width; g.T = (int)T; g.Ts = (int)T | 1;
    const long long tab = (long long)n * g.Ts;
    g.tab_lds = tab <= RS_TAB_LDS;
    const int cap = RS_LDS_FLOATS - (g.tab_lds ? (int)tab : 0);
    int QB = (RS_TILE_OUT + n - 1) / n;
    const int fit = (cap - g.T) / o + 1;
    if (QB > fit) QB = fit;
    g.QB = QB;
    g.span = (QB - 1) * o + g.T;
    return nullptr;
}

inline size_t resample_lds_bytes(const ResampleGeom& g) {
    return ((size_t)g.span + (g.tab_lds ? (size_t)g.n * g.Ts : 0)) * sizeof(float);
}

// Blocks of a stream that are computable after `fed` samples: q < max(0, floor((fed - width - o) / o) + 1)
inline long long ready_blocks(long long fed, int o, int width) {
    const long long a = fed - width - o;
    return a < 0 ? 0 : a / o + 1;
}

}  // namespace

extern "C" int csm_resample_f32(const float* x, const float* taps, float* y, int R, long long N, int o, int n, int width,
                                hipStream_t stream) {
    ResampleGeom g;
    const char* bad = resample_geom(g, o, n, width);
    CSM_REQUIRE(!bad, "csm_resample_f32: %s (o %d, n %d, width %d)", bad, o, n, width);
    CSM_REQUIRE(R >= 1 && R <= 65535 && N >= 0, "csm_resample_f32: R %d rows (1..65535) of N %lld samples", R, N);
    const long long M = ((long long)n * N + o - 1) / o;
    CSM_REQUIRE(N + g.T < (1LL << 31) && M + (long long)g.QB * n < (1LL << 31), "csm_resample_f32: N %lld / M %lld overflow an index", N,
                M);
    if (M == 0) return 0;
    CSM_REQUIRE(x && taps && y, "csm_resample_f32: null pointer");
    const long long blocks = (M + n - 1) / n;
    const unsigned tiles = (unsigned)((blocks + g.QB - 1) / g.QB);
    if (g.tab_lds)
        hipLaunchKernelGGL(resample_kernel<true>, dim3(tiles, R), dim3(RS_THREADS), resample_lds_bytes(g), stream, x, taps, y, g, (int)N,
                           (int)M);
    else
        hipLaunchKernelGGL(resample_kernel<false>, dim3(tiles, R), dim3(RS_THREADS), resample_lds_bytes(g), stream, x, taps, y, g, (int)N,
                           (int)M);
    CSM_CHECK_LAUNCH("csm_resample_f32");
    return 0;
}

extern "C" int csm_resample_stream_rows_f32(float* carry_arena, const float* const* x, const float* taps, float* y, long long ldy, int R,
                                            const int* slots, const int* parity, const int* n_in, const long long* pos,
                                            unsigned final_mask, int n_slots, int max_in, int o, int n, int width, hipStream_t stream) {
    ResampleGeom g;
    const char* bad = resample_geom(g, o, n, width);
    CSM_REQUIRE(!bad, "csm_resample_stream_rows_f32: %s (o %d, n %d, width %d)", bad, o, n, width);
    CSM_REQUIRE(R >= 1 && R <= 16, "csm_resample_stream_rows_f32: R = %d rows (1..16)", R);
    CSM_REQUIRE(slots && parity && n_in && pos && x && n_slots >= 1 && max_in >= 1,
                "csm_resample_stream_rows_f32: null host array, n_slots %d < 1 or max_in %d < 1", n_slots, max_in);
    CSM_REQUIRE((final_mask >> R) == 0, "csm_resample_stream_rows_f32: final mask 0x%x names a row >= R = %d", final_mask, R);
    ResampleRows rows = {};
    const int H = g.T - 1;
    long long max_m = 0;
    for (int r = 0; r < R; ++r) {
        CSM_REQUIRE(slots[r] >= 0 && slots[r] < n_slots, "csm_resample_stream_rows_f32: row %d: slot %d outside [0, %d)", r, slots[r],
                    n_slots);
        for (int q = 0; q < r; ++q)
            CSM_REQUIRE(slots[q] != slots[r], "csm_resample_stream_rows_f32: slot %d is named twice (rows %d and %d)", slots[r], q, r);
        CSM_REQUIRE((parity[r] & ~1) == 0, "csm_resample_stream_rows_f32: row %d: parity %d is not 0 / 1", r, parity[r]);
        const bool fin = (final_mask >> r) & 1u;
        CSM_REQUIRE(n_in[r] >= (fin ? 0 : 1) && n_in[r] <= max_in,
                    "csm_resample_stream_rows_f32: row %d: n_in %d outside 1..max_in = %d (0 only with the row's final bit)", r, n_in[r],
                    max_in);
        CSM_REQUIRE(n_in[r] == 0 || x[r], "csm_resample_stream_rows_f32: row %d: null input", r);
        CSM_REQUIRE(pos[r] >= 0 && pos[r] < (1LL << 62) / n, "csm_resample_stream_rows_f32: row %d: position %lld", r, pos[r]);
        const long long fed = pos[r] + n_in[r];
        const long long q0 = ready_blocks(pos[r], o, width);
        const long long m = fin ? (n * fed + o - 1) / o - n * q0 : n * (ready_blocks(fed, o, width) - q0);
        CSM_REQUIRE(m >= 0 && m <= ldy, "csm_resample_stream_rows_f32: row %d emits %lld outputs, ldy is %lld", r, m, ldy);
        rows.x[r] = x[r];
        rows.slot[r] = slots[r];
        rows.par[r] = parity[r];
        rows.n_in[r] = n_in[r];
        rows.off[r] = (int)(q0 * o - width - (pos[r] - H));           // in [0, H]: the carry reaches back to that block
        rows.m[r] = (int)m;
        if (m > max_m) max_m = m;
    }
    CSM_REQUIRE(carry_arena && taps && (y || max_m == 0), "csm_resample_stream_rows_f32: null pointer");
    CSM_REQUIRE((long long)max_in + 2LL * g.T + (long long)g.QB * o < (1LL << 31) && max_m + (long long)g.QB * n < (1LL << 31),
                "csm_resample_stream_rows_f32: index overflow");
    const long long blocks = (max_m + n - 1) / n;
    unsigned tiles = (unsigned)((blocks + g.QB - 1) / g.QB);
    if (tiles < 1) tiles = 1;                                        // (tile 0 moves the carries on)
    if (g.tab_lds)
        hipLaunchKernelGGL(resample_stream_rows_kernel<true>, dim3(tiles, R), dim3(RS_THREADS), resample_lds_bytes(g), stream, carry_arena,
                           taps, y, rows, g, ldy);
    else
        hipLaunchKernelGGL(resample_stream_rows_kernel<false>, dim3(tiles, R), dim3(RS_THREADS), resample_lds_bytes(g), stream, carry_arena,
                           taps, y, rows, g, ldy);
    CSM_CHECK_LAUNCH("csm_resample_stream_rows_f32");
    return 0;
}

extern "C" int csm_resample_stream_f32(float* carry, int parity, const float* x, int n_in, long long pos, int final, const float* taps,
                                       float* y, long long ldy, int max_in, int o, int n, int width, hipStream_t stream) {
    const int slot = 0;
    return csm_resample_stream_rows_f32(carry, &x, taps, y, ldy, 1, &slot, &parity, &n_in, &pos, final ? 1u : 0u, 1, max_in, o, n, width,
                                        stream);
}
