// Mimi codec kernels for gfx950 (fp32): SEANet causal convolutions / transposed convolutions with fused ELU, bias and
// residual, LayerNorm, a tiled fp32 linear layer with fused GELU / layer-scale / residual epilogues, rotate-half RoPE and
// sliding-window causal attention for the 8-layer codec transformers.
//
// Replaces the moshi 0.2.2 `MimiModel.encode / decode` calls behind reference src/csm/generator.py:67-70,117,209
// (third-party, not vendored; restated from the published architecture and cross-checked against the HF port).
// fp32 on purpose: the encoder ends in a nearest-codeword search whose integer output must match a fp32 CPU run, and the
// whole codec is ~40 GFLOP per 10 s of audio - noise next to the language model - so no MFMA / bf16 here.
#include "common.h"
#include <math.h>

namespace {

// ELU (alpha 1).  expm1f is evaluated for every x and then selected, never branched around: a branch on the loaded value
// would make every load of an unrolled tap loop wait before the next one is issued.
__device__ __forceinline__ float elu1(float x) {
    const float em = expm1f(x);
    return x > 0.f ? x : em;
}

// Per-output accumulations shared by the full-sequence kernels and the streaming ones (csm_*_stream_f32), so that both
// compute every output with the same operations in the same order: a streaming decoder is then bit-identical to decode().

// acc += sum_{ci < cin_g} sum_{j < k} wrow[ci][j] * act(load(ci, j))   (ci outer, j inner)
// The (ci, j) taps run as one flat loop, unrolled so that the loads of several taps are in flight at once: the sum is a
// chain of cin_g * k dependent FMAs whatever the sequence length, and a short (streaming) launch is bound by its latency.
template <class Load>
__device__ __forceinline__ float conv1d_accum(float acc, const float* __restrict__ wrow, int cin_g, int k, int elu_in, Load load) {
    int ci = 0, j = 0;
#pragma unroll 8
    for (int e = 0; e < cin_g * k; ++e) {
        float v = load(ci, j);
        if (elu_in) v = elu1(v);   // ELU(0) = 0, so applying it to zero padding changes nothing
        acc += wrow[e] * v;        // wrow[ci * k + j]
        if (++j == k) { j = 0; ++ci; }
    }
    return acc;
}

// acc += sum_{j = tf % stride, step stride} sum_ci act(load(ci, ti)) w[grp*cin_g + ci][co_g][j], ti = (tf - j) / stride,
// taps with ti outside [0, ti_end) skipped (j outer, ci inner)
template <class Load>
__device__ __forceinline__ float convt_accum(float acc, const float* __restrict__ w, int grp, int cin_g, int cout_g, int co_g, int k,
                                             int stride, int tf, int ti_end, int elu_in, Load load) {
    for (int j = tf % stride; j < k; j += stride) {
        const int ti = (tf - j) / stride;
        if (ti < 0 || ti >= ti_end) continue;
#pragma unroll 8
        for (int ci = 0; ci < cin_g; ++ci) {
            float v = load(ci, ti);
            if (elu_in) v = elu1(v);
            acc += v * w[((size_t)(grp * cin_g + ci) * cout_g + co_g) * k + j];
        }
    }
    return acc;
}

// y[co][t] = bias[co] + sum_{ci in group} sum_j w[co][ci][j] * act(xpad[ci][t*stride + j*dil - pad_left]) (+ res[co][t])
// xpad: zero (pad_mode 0) or edge-replicated (pad_mode 1) outside [0, T_in).  One wave-row of threads shares `co`, so the
// weights are wave-uniform (scalar loads) and the input reads are coalesced along time.
__global__ __launch_bounds__(256) void conv1d_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ res,
                                                     float* __restrict__ y, int C_in, int C_out, int T_in, int T_out, int k,
                                                     int stride, int dil, int pad_left, int pad_mode, int groups, int elu_in) {
    const int co = blockIdx.y;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g;
    const float* wrow = w + (size_t)co * cin_g * k;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T_out; t += gridDim.x * blockDim.x) {
        const int base = t * stride - pad_left;
        float acc = conv1d_accum(bias ? bias[co] : 0.f, wrow, cin_g, k, elu_in, [&](int ci, int j) {
            const float* xr = x + (size_t)(grp * cin_g + ci) * T_in;
            const int p = base + j * dil;
            if (p >= 0 && p < T_in) return xr[p];
            if (pad_mode == 1) return xr[p < 0 ? 0 : T_in - 1];
            return 0.f;
        });
        if (res) acc += res[(size_t)co * T_out + t];
        y[(size_t)co * T_out + t] = acc;
    }
}

// Streaming causal stride-1 conv: the input is [hist | x] with hist = the last H = (k-1)*dil input columns of the previous
// chunk (zeros before the first: decode()'s zero padding).  Writes y[co][0..n) as conv1d_kernel does for the same absolute
// outputs, and the next history (the last H columns of [hist | x]) into hist_out - a different buffer (the host ping-pongs).
__global__ __launch_bounds__(256) void conv1d_stream_kernel(const float* __restrict__ hist, const float* __restrict__ x,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ res, float* __restrict__ y,
                                                            float* __restrict__ hist_out, int C_in, int C_out, int n, int k, int dil,
                                                            int groups, int elu_in) {
    const int co = blockIdx.y;
    const int H = (k - 1) * dil;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g;
    const float* wrow = w + (size_t)co * cin_g * k;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        float acc = conv1d_accum(bias ? bias[co] : 0.f, wrow, cin_g, k, elu_in, [&](int ci, int j) {
            const int c = grp * cin_g + ci, p = t + j * dil;            // column of [hist | x]
            // select the address, then load unconditionally: a load under a branch cannot be hoisted out of the unrolled loop
            const float* src = p < H ? hist + (size_t)c * H + p : x + (size_t)c * n + (p - H);
            return *src;
        });
        if (res) acc += res[(size_t)co * n + t];
        y[(size_t)co * n + t] = acc;
    }
    for (int c = blockIdx.y; c < C_in; c += gridDim.y)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H; i += gridDim.x * blockDim.x) {
            const int p = n + i;
            hist_out[(size_t)c * H + i] = p < H ? hist[(size_t)c * H + p] : x[(size_t)c * n + p - H];
        }
}

// Streaming causal conv with stride >= 1 (the encoder's downsampling layers): the input is [hist | x] with x = n_in new
// columns (a multiple of stride) and hist = the last H = (k-1)*dil + 1 - stride input columns before them - conv1d_kernel's
// pad_left, zeros before the first chunk.  Output t of the chunk starts at column t*stride of [hist | x]; it goes through
// conv1d_accum with the operands conv1d_kernel reads for the same absolute output.  edge_first (the first chunk of an
// edge-replicated conv, pad_mode 1): hist is not read, every history column is column 0 of x.  The next history is the last
// H columns of [hist | x]; H may exceed n_in, then it keeps H - n_in old columns.  Time is flattened onto the threads of one
// output channel as in conv1d_kernel: the early encoder layers carry hundreds of columns per frame.
__global__ __launch_bounds__(256) void conv1d_stream_strided_kernel(const float* __restrict__ hist, const float* __restrict__ x,
                                                                    const float* __restrict__ w, const float* __restrict__ bias,
                                                                    const float* __restrict__ res, float* __restrict__ y,
                                                                    float* __restrict__ hist_out, int C_in, int C_out, int n_in, int k,
                                                                    int stride, int dil, int groups, int elu_in, int edge_first) {
    const int co = blockIdx.y;
    const int H = (k - 1) * dil + 1 - stride;
    const int n_out = n_in / stride;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g;
    const float* wrow = w + (size_t)co * cin_g * k;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_out; t += gridDim.x * blockDim.x) {
        const int base = t * stride;
        float acc = conv1d_accum(bias ? bias[co] : 0.f, wrow, cin_g, k, elu_in, [&](int ci, int j) {
            const int c = grp * cin_g + ci, p = base + j * dil;         // column of [hist | x]
            const float* xr = x + (size_t)c * n_in;
            // select the address, then load unconditionally (as conv1d_stream_kernel)
            const float* old = edge_first ? xr : hist + (size_t)c * H + p;
            const float* src = p < H ? old : xr + (p - H);
            return *src;
        });
        if (res) acc += res[(size_t)co * n_out + t];
        y[(size_t)co * n_out + t] = acc;
    }
    for (int c = blockIdx.y; c < C_in; c += gridDim.y)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H; i += gridDim.x * blockDim.x) {
            const int p = n_in + i;
            const float* xr = x + (size_t)c * n_in;
            const float* old = edge_first ? xr : hist + (size_t)c * H + p;
            hist_out[(size_t)c * H + i] = *(p < H ? old : xr + (p - H));
        }
}

// ConvTranspose1d (torch weight layout [C_in][C_out/groups][k]) cropped to [crop_left, crop_left + T_out):
// y[co][t] = bias[co] + sum_ci sum_{j : (t + crop_left - j) % stride == 0} act(x[ci][(t + crop_left - j)/stride]) w[ci][co_g][j]
__global__ __launch_bounds__(256) void conv_transpose1d_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ y, int C_in,
                                                               int C_out, int T_in, int T_out, int k, int stride, int crop_left,
                                                               int groups, int elu_in) {
    const int co = blockIdx.y;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g, co_g = co % cout_g;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T_out; t += gridDim.x * blockDim.x) {
        const float acc = convt_accum(bias ? bias[co] : 0.f, w, grp, cin_g, cout_g, co_g, k, stride, t + crop_left, T_in, elu_in,
                                      [&](int ci, int ti) { return x[(size_t)(grp * cin_g + ci) * T_in + ti]; });
        y[(size_t)co * T_out + t] = acc;
    }
}

// Streaming causal (crop_left 0) transposed conv: chunk of n input columns at absolute input position pos0, history = the last
// H = ceil(k/stride) - 1 input columns before it.  Writes the n*stride outputs that conv_transpose1d_kernel gives for absolute
// outputs [pos0*stride, (pos0+n)*stride) - the taps of inputs before position 0 are skipped, as there - and the next history.
__global__ __launch_bounds__(256) void conv_transpose1d_stream_kernel(const float* __restrict__ hist, const float* __restrict__ x,
                                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                                      float* __restrict__ y, float* __restrict__ hist_out, int C_in,
                                                                      int C_out, int n, int pos0, int k, int stride, int groups,
                                                                      int elu_in) {
    const int co = blockIdx.y;
    const int H = (k - 1) / stride;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g, co_g = co % cout_g;
    const int T_out = n * stride;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T_out; t += gridDim.x * blockDim.x) {
        const float acc = convt_accum(bias ? bias[co] : 0.f, w, grp, cin_g, cout_g, co_g, k, stride, pos0 * stride + t, pos0 + n, elu_in,
                                      [&](int ci, int ti) {
                                          const int c = grp * cin_g + ci, p = ti - pos0 + H;      // column of [hist | x]
                                          const float* src = p < H ? hist + (size_t)c * H + p : x + (size_t)c * n + (p - H);
                                          return *src;
                                      });
        y[(size_t)co * T_out + t] = acc;
    }
    for (int c = blockIdx.y; c < C_in; c += gridDim.y)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H; i += gridDim.x * blockDim.x) {
            const int p = n + i;
            hist_out[(size_t)c * H + i] = p < H ? hist[(size_t)c * H + p] : x[(size_t)c * n + p - H];
        }
}

// y[t][:] = (x[t] - mean) * rsqrt(var + eps) * w + b      (one wave per row)
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* __restrict__ y, int T, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= T) return;
    const float* xr = x + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += xr[c];
    const float mean = wave_sum(s) / D;
    float v = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = xr[c] - mean; v += d * d; }
    const float r = rsqrtf(wave_sum(v) / D + eps);
    for (int c = lane; c < D; c += 64) y[(size_t)row * D + c] = (xr[c] - mean) * r * w[c] + b[c];
}

// act 1 = exact GELU; scale != NULL -> res + scale[n] * v (layer scale + residual); else v (+ res)
__device__ __forceinline__ float linear_epilogue(float v, const float* __restrict__ scale, const float* __restrict__ res, int t, int n,
                                                 int N, int act) {
    if (act == 1) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
    if (scale) v = res[(size_t)t * N + n] + scale[n] * v;
    else if (res) v += res[(size_t)t * N + n];
    return v;
}

// y[T][N] = epilogue(x[T][K] W[N][K]^T): 64x64 tile per 256-thread block, 4x4 outputs per thread, K in steps of 16
// epilogue: act 1 = exact GELU; scale != NULL -> y = res + scale[n] * acc (layer scale + residual); else y = acc (+ res)
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ scale, const float* __restrict__ res,
                                                         float* __restrict__ y, int T, int N, int K, int ldx, int act) {
    __shared__ float xs[16][64 + 1], ws[16][64 + 1];
    const int t0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;       // 16 x 16 threads, each 4 (t) x 4 (n)
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            const int r = i >> 4, c = i & 15;
            xs[c][r] = (t0 + r < T && k0 + c < K) ? x[(size_t)(t0 + r) * ldx + k0 + c] : 0.f;
            ws[c][r] = (n0 + r < N && k0 + c < K) ? W[(size_t)(n0 + r) * K + k0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = xs[c][ty * 4 + i]; b[i] = ws[c][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + ty * 4 + i;
        if (t >= T) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= N) continue;
            y[(size_t)t * N + n] = linear_epilogue(acc[i][j], scale, res, t, n, N, act);
        }
    }
}

// linear_f32_kernel's products for a few rows (the streaming decoder's 2n positions): one thread per output, the same
// k-ascending chain of FMAs from 0 and the same epilogue, so every output has the tiled kernel's bits.  The tiled kernel
// pays a global -> LDS round trip and two barriers per 16 k on only N/64 blocks; here each thread streams its weight row
// with 16-byte loads, the next V float4 in flight while the current V are consumed.  Needs K % (4 V) == 0, W 16-B aligned.
template <int V>
__global__ __launch_bounds__(256) void linear_f32_rows_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                              const float* __restrict__ scale, const float* __restrict__ res,
                                                              float* __restrict__ y, int T, int N, int K, int ldx, int act) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (n >= N) return;
    const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)n * K);
    const float* xr = x + (size_t)t * ldx;
    const int nb = K / (4 * V);
    float4 cur[V], nxt[V];
#pragma unroll
    for (int v = 0; v < V; ++v) cur[v] = w4[v];
    float acc = 0.f;
    for (int b = 0; b < nb; ++b) {
        if (b + 1 < nb) {
#pragma unroll
            for (int v = 0; v < V; ++v) nxt[v] = w4[(b + 1) * V + v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float* xk = xr + (b * V + v) * 4;
            acc = fmaf(xk[0], cur[v].x, acc);
            acc = fmaf(xk[1], cur[v].y, acc);
            acc = fmaf(xk[2], cur[v].z, acc);
            acc = fmaf(xk[3], cur[v].w, acc);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) cur[v] = nxt[v];
    }
    y[(size_t)t * N + n] = linear_epilogue(acc, scale, res, t, n, N, act);
}

// rotate-half RoPE (HF / moshi convention) in place on the q and k parts of qkv [T][3*H*hd]; theta_i = base^(-2i/hd)
__global__ __launch_bounds__(256) void rope_half_kernel(float* __restrict__ qkv, int T, int H, int hd, float base, int pos0) {
    const int half = hd >> 1;
    const long long total = (long long)T * 2 * H * half;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(idx % half);
        const int hh = (int)((idx / half) % (2 * H));          // q heads then k heads
        const int t = (int)(idx / ((long long)half * 2 * H));
        const float inv = powf(base, -2.f * i / hd);
        float sn, cs;
        sincosf((float)(pos0 + t) * inv, &sn, &cs);
        float* p = qkv + (size_t)t * 3 * H * hd + (size_t)hh * hd;
        const float a = p[i], b = p[i + half];
        float ra = a, rb = b;
        rope_rot(ra, rb, cs, sn);
        p[i] = ra;
        p[i + half] = rb;
    }
}

// One query row of causal sliding-window attention over n keys: key s (logical order) on lane s % 64, row pointers from
// krow(s) / vrow(s); sc = LDS scores [n].  Shared by the full-sequence and the streaming kernel.
template <int HD, class KRow, class VRow>
__device__ __forceinline__ void attn_window_row(const float* __restrict__ qp, float* __restrict__ outp, float* sc, int n, int lane,
                                                KRow krow, VRow vrow) {
    const float scale = rsqrtf((float)HD);
    float mx = -INFINITY;
    for (int s = lane; s < n; s += 64) {
        const float* kp = krow(s);
        float d = 0.f;
#pragma unroll 8
        for (int c = 0; c < HD; ++c) d += qp[c] * kp[c];
        d *= scale;
        sc[s] = d;
        mx = fmaxf(mx, d);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int s = lane; s < n; s += 64) { const float p = expf(sc[s] - mx); sc[s] = p; sum += p; }
    sum = wave_sum(sum);
    __syncthreads();
    for (int c = lane; c < HD; c += 64) {
        float acc = 0.f;
        for (int s = 0; s < n; ++s) acc += sc[s] * vrow(s)[c];
        outp[c] = acc / sum;
    }
}

// causal sliding-window attention, one block per (query, head); keys in (q - window, q]
template <int HD>
__global__ __launch_bounds__(64) void attn_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, int H, int window) {
    extern __shared__ float sc[];   // [window]
    const int q = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int ld = 3 * H * HD;
    const int k_lo = q - window + 1 > 0 ? q - window + 1 : 0;
    attn_window_row<HD>(qkv + (size_t)q * ld + h * HD, out + (size_t)q * H * HD + h * HD, sc, q - k_lo + 1, lane,
                        [&](int s) { return qkv + (size_t)(k_lo + s) * ld + (H + h) * HD; },
                        [&](int s) { return qkv + (size_t)(k_lo + s) * ld + (2 * H + h) * HD; });
}

// The same for n new rows of qkv at absolute positions pos0 .. pos0+n-1.  Keys before pos0 come from the K/V ring caches
// ([ring][H*HD], position p in slot p % ring, post-RoPE), the chunk's own keys straight from qkv; block (q, h) also appends
// its k / v head row to slot (pos0 + q) % ring.  The slots written, (pos0 .. pos0+n-1), and the slots read from the cache,
// (pos0-window+1 .. pos0-1), are n + window - 1 consecutive positions: distinct when ring >= window + n - 1 (checked by the
// host wrapper), so no block overwrites a key another block of the launch still reads.  A ring of exactly `window` slots
// would not do: the slot of new position p holds p - window, which earlier queries of the same chunk still need.
template <int HD>
__global__ __launch_bounds__(64) void attn_f32_stream_kernel(const float* __restrict__ qkv, float* __restrict__ kc, float* __restrict__ vc,
                                                             float* __restrict__ out, int pos0, int H, int window, int ring) {
    extern __shared__ float sc[];   // [window]
    const int qi = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int ld = 3 * H * HD, ldc = H * HD;
    const int q = pos0 + qi;
    const size_t slot = (size_t)(q % ring) * ldc + h * HD;
    for (int c = lane; c < HD; c += 64) {
        kc[slot + c] = qkv[(size_t)qi * ld + (H + h) * HD + c];
        vc[slot + c] = qkv[(size_t)qi * ld + (2 * H + h) * HD + c];
    }
    const int k_lo = q - window + 1 > 0 ? q - window + 1 : 0;
    attn_window_row<HD>(qkv + (size_t)qi * ld + h * HD, out + (size_t)qi * H * HD + h * HD, sc, q - k_lo + 1, lane,
                        [&](int s) {
                            const int p = k_lo + s;
                            return p >= pos0 ? qkv + (size_t)(p - pos0) * ld + (H + h) * HD : kc + (size_t)(p % ring) * ldc + h * HD;
                        },
                        [&](int s) {
                            const int p = k_lo + s;
                            return p >= pos0 ? qkv + (size_t)(p - pos0) * ld + (2 * H + h) * HD : vc + (size_t)(p % ring) * ldc + h * HD;
                        });
}

// out[b][c][r] = in[b][r][c], b = blockIdx.z (one matrix: a grid of depth 1)
__global__ __launch_bounds__(256) void transpose_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int Cn) {
    __shared__ float tile[32][33];
    in += (size_t)blockIdx.z * R * Cn;
    out += (size_t)blockIdx.z * R * Cn;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && c0 + tx < Cn) tile[i][tx] = in[(size_t)(r0 + i) * Cn + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < Cn && r0 + tx < R) out[(size_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

// ---- rows forms of the streaming ops: R <= 16 utterances, each with its own state slot, decoded or encoded by one launch ---
// (the decoder's: stride-1 conv, transposed conv, RoPE, ring attention, transpose; the encoder's adds the strided conv)
// A streaming step is a chain of dependent FMAs per output with nothing to overlap, and a 4-frame chunk fills 8 lanes of a
// wave in the wide early layers; the rows of a batch are the missing parallelism.  The launches below flatten (row, time)
// onto the threads of one output channel - the weights stay wave-uniform - and every output goes through conv1d_accum /
// convt_accum / attn_window_row with the operands of the one-row stream kernel, so a row has that kernel's bits.
// The per-row slot, history parity and position travel by value in the kernel arguments: no device buffer, no copy, no sync.
struct StreamRows {
    int slot[16];   // state slot of row r (index into the arenas' leading dimension)
    int par[16];    // which of the slot's two history buffers holds the current history (the other receives the next)
    int pos[16];    // absolute position of the row's first new input column / transformer row
};

// x [R][C_in][n], y / res [R][C_out][n], hist arena [slots][2][C_in][H].  k == 1: H == 0 and the arena is NULL - the history
// pointers formed from it below are then never dereferenced (no column p < H exists, and the history loop has no iteration).
__global__ __launch_bounds__(256) void conv1d_stream_rows_kernel(float* __restrict__ arena, const float* __restrict__ x,
                                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                                 const float* __restrict__ res, float* __restrict__ y, StreamRows rows,
                                                                 int R, int C_in, int C_out, int n, int k, int dil, int groups,
                                                                 int elu_in) {
    const int co = blockIdx.y;
    const int H = (k - 1) * dil;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g;
    const float* wrow = w + (size_t)co * cin_g * k;
    const size_t hsz = (size_t)C_in * H;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < R * n; g += gridDim.x * blockDim.x) {
        const int r = g / n, t = g - r * n;
        const float* hist = arena + ((size_t)rows.slot[r] * 2 + rows.par[r]) * hsz;
        const float* xr = x + (size_t)r * C_in * n;
        float acc = conv1d_accum(bias ? bias[co] : 0.f, wrow, cin_g, k, elu_in, [&](int ci, int j) {
            const int c = grp * cin_g + ci, p = t + j * dil;            // column of [hist | x]
            const float* src = p < H ? hist + (size_t)c * H + p : xr + (size_t)c * n + (p - H);
            return *src;
        });
        const size_t o = ((size_t)r * C_out + co) * n + t;
        if (res) acc += res[o];
        y[o] = acc;
    }
    for (int c = blockIdx.y; c < C_in; c += gridDim.y)
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < R * H; g += gridDim.x * blockDim.x) {
            const int r = g / H, i = g - r * H;
            const float* hist = arena + ((size_t)rows.slot[r] * 2 + rows.par[r]) * hsz;
            float* hist_out = arena + ((size_t)rows.slot[r] * 2 + (rows.par[r] ^ 1)) * hsz;
            const int p = n + i;
            hist_out[(size_t)c * H + i] = p < H ? hist[(size_t)c * H + p] : x[((size_t)r * C_in + c) * n + p - H];
        }
}

// conv1d_stream_strided_kernel for R rows: x [R][C_in][n_in], y / res [R][C_out][n_in / stride], hist arena [slots][2][C_in][H]
// with H = (k-1)*dil + 1 - stride.  Bit r of edge_mask = row r is the first chunk of an edge-replicated conv: its history is not
// read, every history column is column 0 of its x.  The flag differs between the lanes of a wave, so it only selects an address;
// the load stays unconditional.  H == 0: NULL arena, never dereferenced - as above.
__global__ __launch_bounds__(256) void conv1d_stream_strided_rows_kernel(float* __restrict__ arena, const float* __restrict__ x,
                                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                                         const float* __restrict__ res, float* __restrict__ y,
                                                                         StreamRows rows, unsigned edge_mask, int R, int C_in, int C_out,
                                                                         int n_in, int k, int stride, int dil, int groups, int elu_in) {
    const int co = blockIdx.y;
    const int H = (k - 1) * dil + 1 - stride;
    const int n_out = n_in / stride;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g;
    const float* wrow = w + (size_t)co * cin_g * k;
    const size_t hsz = (size_t)C_in * H;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < R * n_out; g += gridDim.x * blockDim.x) {
        const int r = g / n_out, t = g - r * n_out;
        const int base = t * stride;
        const bool edge = (edge_mask >> r) & 1u;
        const float* hist = arena + ((size_t)rows.slot[r] * 2 + rows.par[r]) * hsz;
        const float* xrow = x + (size_t)r * C_in * n_in;
        float acc = conv1d_accum(bias ? bias[co] : 0.f, wrow, cin_g, k, elu_in, [&](int ci, int j) {
            const int c = grp * cin_g + ci, p = base + j * dil;         // column of [hist | x]
            const float* xr = xrow + (size_t)c * n_in;
            const float* old = edge ? xr : hist + (size_t)c * H + p;
            const float* src = p < H ? old : xr + (p - H);
            return *src;
        });
        const size_t o = ((size_t)r * C_out + co) * n_out + t;
        if (res) acc += res[o];
        y[o] = acc;
    }
    for (int c = blockIdx.y; c < C_in; c += gridDim.y)
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < R * H; g += gridDim.x * blockDim.x) {
            const int r = g / H, i = g - r * H;
            const float* hist = arena + ((size_t)rows.slot[r] * 2 + rows.par[r]) * hsz;
            float* hist_out = arena + ((size_t)rows.slot[r] * 2 + (rows.par[r] ^ 1)) * hsz;
            const int p = n_in + i;
            const float* xr = x + ((size_t)r * C_in + c) * n_in;
            const float* old = ((edge_mask >> r) & 1u) ? xr : hist + (size_t)c * H + p;
            hist_out[(size_t)c * H + i] = *(p < H ? old : xr + (p - H));
        }
}

// x [R][C_in][n], y [R][C_out][n*stride], hist arena [slots][2][C_in][H]; rows.pos = absolute input position of column 0
// (k <= stride: H == 0, NULL arena, never dereferenced - as above)
__global__ __launch_bounds__(256) void conv_transpose1d_stream_rows_kernel(float* __restrict__ arena, const float* __restrict__ x,
                                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                                           float* __restrict__ y, StreamRows rows, int R, int C_in,
                                                                           int C_out, int n, int k, int stride, int groups, int elu_in) {
    const int co = blockIdx.y;
    const int H = (k - 1) / stride;
    const int cin_g = C_in / groups, cout_g = C_out / groups;
    const int grp = co / cout_g, co_g = co % cout_g;
    const int T_out = n * stride;
    const size_t hsz = (size_t)C_in * H;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < R * T_out; g += gridDim.x * blockDim.x) {
        const int r = g / T_out, t = g - r * T_out;
        const int pos0 = rows.pos[r];
        const float* hist = arena + ((size_t)rows.slot[r] * 2 + rows.par[r]) * hsz;
        const float* xr = x + (size_t)r * C_in * n;
        const float acc = convt_accum(bias ? bias[co] : 0.f, w, grp, cin_g, cout_g, co_g, k, stride, pos0 * stride + t, pos0 + n, elu_in,
                                      [&](int ci, int ti) {
                                          const int c = grp * cin_g + ci, p = ti - pos0 + H;      // column of [hist | x]
                                          const float* src = p < H ? hist + (size_t)c * H + p : xr + (size_t)c * n + (p - H);
                                          return *src;
                                      });
        y[((size_t)r * C_out + co) * T_out + t] = acc;
    }
    for (int c = blockIdx.y; c < C_in; c += gridDim.y)
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < R * H; g += gridDim.x * blockDim.x) {
            const int r = g / H, i = g - r * H;
            const float* hist = arena + ((size_t)rows.slot[r] * 2 + rows.par[r]) * hsz;
            float* hist_out = arena + ((size_t)rows.slot[r] * 2 + (rows.par[r] ^ 1)) * hsz;
            const int p = n + i;
            hist_out[(size_t)c * H + i] = p < H ? hist[(size_t)c * H + p] : x[((size_t)r * C_in + c) * n + p - H];
        }
}

// rope_half_kernel on qkv [R*n][3*H*hd]: row r's n positions start at rows.pos[r]
__global__ __launch_bounds__(256) void rope_half_rows_kernel(float* __restrict__ qkv, StreamRows rows, int R, int n, int H, int hd,
                                                             float base) {
    const int half = hd >> 1;
    const long long total = (long long)R * n * 2 * H * half;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(idx % half);
        const int hh = (int)((idx / half) % (2 * H));          // q heads then k heads
        const int tg = (int)(idx / ((long long)half * 2 * H));
        const int r = tg / n, t = tg - r * n;
        const float inv = powf(base, -2.f * i / hd);
        float sn, cs;
        sincosf((float)(rows.pos[r] + t) * inv, &sn, &cs);
        float* p = qkv + (size_t)tg * 3 * H * hd + (size_t)hh * hd;
        const float a = p[i], b = p[i + half];
        float ra = a, rb = b;
        rope_rot(ra, rb, cs, sn);
        p[i] = ra;
        p[i + half] = rb;
    }
}

// attn_f32_stream_kernel for R rows: qkv [R*n][3*H*HD], out [R*n][H*HD], K/V ring arenas [slots][ring][H*HD]; block (q, h, r)
template <int HD>
__global__ __launch_bounds__(64) void attn_f32_stream_rows_kernel(const float* __restrict__ qkv_all, float* __restrict__ kc_all,
                                                                  float* __restrict__ vc_all, float* __restrict__ out_all, StreamRows rows,
                                                                  int n, int H, int window, int ring) {
    extern __shared__ float sc[];   // [window]
    const int qi = blockIdx.x, h = blockIdx.y, r = blockIdx.z, lane = threadIdx.x;
    const int ld = 3 * H * HD, ldc = H * HD;
    const int pos0 = rows.pos[r];
    const float* qkv = qkv_all + (size_t)r * n * ld;
    float* kc = kc_all + (size_t)rows.slot[r] * ring * ldc;
    float* vc = vc_all + (size_t)rows.slot[r] * ring * ldc;
    float* out = out_all + (size_t)r * n * ldc;
    const int q = pos0 + qi;
    const size_t slot = (size_t)(q % ring) * ldc + h * HD;
    for (int c = lane; c < HD; c += 64) {
        kc[slot + c] = qkv[(size_t)qi * ld + (H + h) * HD + c];
        vc[slot + c] = qkv[(size_t)qi * ld + (2 * H + h) * HD + c];
    }
    const int k_lo = q - window + 1 > 0 ? q - window + 1 : 0;
    attn_window_row<HD>(qkv + (size_t)qi * ld + h * HD, out + (size_t)qi * H * HD + h * HD, sc, q - k_lo + 1, lane,
                        [&](int s) {
                            const int p = k_lo + s;
                            return p >= pos0 ? qkv + (size_t)(p - pos0) * ld + (H + h) * HD : kc + (size_t)(p % ring) * ldc + h * HD;
                        },
                        [&](int s) {
                            const int p = k_lo + s;
                            return p >= pos0 ? qkv + (size_t)(p - pos0) * ld + (2 * H + h) * HD : vc + (size_t)(p % ring) * ldc + h * HD;
                        });
}

// Host lists (R ints each) -> the by-value argument; false when a slot is out of range or named twice (two rows of one launch
// would write the same state) or a parity is not 0 / 1.
bool stream_rows_arg(StreamRows& a, int R, const int* slots, const int* parity, const int* pos0, int n_slots) {
    if (R < 1 || R > 16 || !slots || n_slots < 1) return false;
    for (int r = 0; r < 16; ++r) a.slot[r] = a.par[r] = a.pos[r] = 0;
    for (int r = 0; r < R; ++r) {
        if (slots[r] < 0 || slots[r] >= n_slots) return false;
        for (int q = 0; q < r; ++q)
            if (slots[q] == slots[r]) return false;
        if (parity && (parity[r] & ~1)) return false;
        if (pos0 && pos0[r] < 0) return false;
        a.slot[r] = slots[r];
        a.par[r] = parity ? parity[r] : 0;
        a.pos[r] = pos0 ? pos0[r] : 0;
    }
    return true;
}

// threads for `work` items of one output channel: whole waves, at most 256
inline int rows_block(long long work) { return work >= 256 ? 256 : (int)((work + 63) / 64) * 64; }

}  // namespace

extern "C" int csm_conv1d_stream_rows_f32(float* hist_arena, const float* x, const float* w, const float* bias, const float* residual,
                                          float* y, int R, const int* slots, const int* parity, int n_slots, int C_in, int C_out, int n,
                                          int k, int dilation, int groups, int elu_in, hipStream_t stream) {
    CSM_REQUIRE(x && w && y && C_in > 0 && C_out > 0 && n > 0 && k > 0 && dilation > 0 && groups > 0 && C_in % groups == 0 &&
                    C_out % groups == 0 && C_out <= 65535, "csm_conv1d_stream_rows_f32: bad arguments");
    CSM_REQUIRE(k == 1 || (hist_arena && parity), "csm_conv1d_stream_rows_f32: k > 1 needs the history arena and the rows' parities");
    StreamRows rows;
    CSM_REQUIRE(stream_rows_arg(rows, R, slots, parity, nullptr, n_slots),
                "csm_conv1d_stream_rows_f32: 1..16 rows with distinct slots in [0, %d) and parities 0 / 1", n_slots);
    const int bs = rows_block((long long)R * n);
    int bx = (int)(((long long)R * n + bs - 1) / bs);
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(conv1d_stream_rows_kernel, dim3(bx, C_out), dim3(bs), 0, stream, hist_arena, x, w, bias, residual, y, rows, R, C_in,
                       C_out, n, k, dilation, groups, elu_in);
    CSM_CHECK_LAUNCH("csm_conv1d_stream_rows_f32");
    return 0;
}

extern "C" int csm_conv1d_stream_strided_rows_f32(float* hist_arena, const float* x, const float* w, const float* bias,
                                                  const float* residual, float* y, int R, const int* slots, const int* parity,
                                                  unsigned edge_first_mask, int n_slots, int C_in, int C_out, int n_in, int k, int stride,
                                                  int dilation, int groups, int elu_in, hipStream_t stream) {
    CSM_REQUIRE(x && w && y && C_in > 0 && C_out > 0 && n_in > 0 && k > 0 && stride > 0 && dilation > 0 && groups > 0 &&
                    C_in % groups == 0 && C_out % groups == 0 && C_out <= 65535, "csm_conv1d_stream_strided_rows_f32: bad arguments");
    CSM_REQUIRE(n_in % stride == 0, "csm_conv1d_stream_strided_rows_f32: n_in %d is not a multiple of stride %d", n_in, stride);
    const long long H = (long long)(k - 1) * dilation + 1 - stride;
    CSM_REQUIRE(H >= 0, "csm_conv1d_stream_strided_rows_f32: stride %d exceeds the kernel's extent (k %d, dilation %d)", stride, k,
                dilation);
    CSM_REQUIRE(H == 0 || (hist_arena && parity),
                "csm_conv1d_stream_strided_rows_f32: a history of %lld columns needs the history arena and the rows' parities", H);
    StreamRows rows;
    CSM_REQUIRE(stream_rows_arg(rows, R, slots, parity, nullptr, n_slots),
                "csm_conv1d_stream_strided_rows_f32: 1..16 rows with distinct slots in [0, %d) and parities 0 / 1", n_slots);
    CSM_REQUIRE((edge_first_mask >> R) == 0,"csm_conv1d_stream_strided_rows_f32: edge-first mask 0x%x names a row >= R = %d",
                edge_first_mask, R);
    const int n_out = n_in / stride;
    CSM_REQUIRE(H + n_in < (1LL << 31) && 16 * H < (1LL << 31) && 16LL * n_out < (1LL << 31),
                "csm_conv1d_stream_strided_rows_f32: column index overflow");
    const long long work = (long long)R * (n_out > H ? n_out : H);   // the same grid writes the outputs and the next histories
    const int bs = rows_block(work);
    long long bx = (work + bs - 1) / bs;
    if (bx > 4096) bx = 4096;                                        // 16 rows x 32 frames x 1920 columns = 3840 blocks of 256
    hipLaunchKernelGGL(conv1d_stream_strided_rows_kernel, dim3((unsigned)bx, C_out), dim3(bs), 0, stream, hist_arena, x, w, bias, residual,
                       y, rows, edge_first_mask, R, C_in, C_out, n_in, k, stride, dilation, groups, elu_in);
    CSM_CHECK_LAUNCH("csm_conv1d_stream_strided_rows_f32");
    return 0;
}

extern "C" int csm_conv_transpose1d_stream_rows_f32(float* hist_arena, const float* x, const float* w, const float* bias, float* y, int R,
                                                    const int* slots, const int* parity, const int* pos0, int n_slots, int C_in,
                                                    int C_out, int n, int k, int stride, int groups, int elu_in, hipStream_t stream) {
    CSM_REQUIRE(x && w && y && pos0 && C_in > 0 && C_out > 0 && n > 0 && k > 0 && stride > 0 && groups > 0 && C_in % groups == 0 &&
                    C_out % groups == 0 && C_out <= 65535, "csm_conv_transpose1d_stream_rows_f32: bad arguments");
    CSM_REQUIRE(k <= stride || (hist_arena && parity),
                "csm_conv_transpose1d_stream_rows_f32: k > stride needs the history arena and the rows' parities");
    StreamRows rows;
    CSM_REQUIRE(stream_rows_arg(rows, R, slots, parity, pos0, n_slots),
                "csm_conv_transpose1d_stream_rows_f32: 1..16 rows with distinct slots in [0, %d), parities 0 / 1, positions >= 0", n_slots);
    for (int r = 0; r < R; ++r)
        CSM_REQUIRE(((long long)pos0[r] + n) * stride < (1LL << 31), "csm_conv_transpose1d_stream_rows_f32: position overflow");
    const long long work = (long long)R * n * stride;
    const int bs = rows_block(work);
    long long bx = (work + bs - 1) / bs;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(conv_transpose1d_stream_rows_kernel, dim3((unsigned)bx, C_out), dim3(bs), 0, stream, hist_arena, x, w, bias, y, rows,
                       R, C_in, C_out, n, k, stride, groups, elu_in);
    CSM_CHECK_LAUNCH("csm_conv_transpose1d_stream_rows_f32");
    return 0;
}

extern "C" int csm_rope_half_rows_f32(float* qkv, int R, const int* pos0, int n, int H, int head_dim, float base, hipStream_t stream) {
    CSM_REQUIRE(qkv && pos0 && R >= 1 && R <= 16 && n > 0 && H > 0 && head_dim > 0 && (head_dim & 1) == 0,
                "csm_rope_half_rows_f32: bad arguments");
    StreamRows rows = {};
    for (int r = 0; r < R; ++r) {
        CSM_REQUIRE(pos0[r] >= 0 && (long long)pos0[r] + n < (1LL << 31), "csm_rope_half_rows_f32: bad position");
        rows.pos[r] = pos0[r];
    }
    const long long total = (long long)R * n * 2 * H * (head_dim / 2);
    long long b = (total + 255) / 256;
    hipLaunchKernelGGL(rope_half_rows_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, stream, qkv, rows, R, n, H, head_dim,
                       base);
    CSM_CHECK_LAUNCH("csm_rope_half_rows_f32");
    return 0;
}

extern "C" int csm_attn_window_stream_rows_f32(const float* qkv, float* kcache, float* vcache, float* out, int R, const int* slots,
                                               const int* pos0, int n_slots, int n, int H, int head_dim, int window, int ring,
                                               hipStream_t stream) {
    CSM_REQUIRE(qkv && kcache && vcache && out && pos0 && n > 0 && H > 0 && window > 0 && window <= 8192 && n <= 65535 && H <= 65535,
                "csm_attn_window_stream_rows_f32: bad arguments");
    CSM_REQUIRE(ring >= window + n - 1, "csm_attn_window_stream_rows_f32: ring %d < window %d + n %d - 1", ring, window, n);
    CSM_REQUIRE(head_dim == 64, "csm_attn_window_stream_rows_f32: head_dim %d unsupported (64)", head_dim);
    StreamRows rows;
    CSM_REQUIRE(stream_rows_arg(rows, R, slots, nullptr, pos0, n_slots),
                "csm_attn_window_stream_rows_f32: 1..16 rows with distinct slots in [0, %d) and positions >= 0", n_slots);
    for (int r = 0; r < R; ++r)
        CSM_REQUIRE((long long)pos0[r] + n < (1LL << 31), "csm_attn_window_stream_rows_f32: position overflow");
    hipLaunchKernelGGL((attn_f32_stream_rows_kernel<64>), dim3(n, H, R), dim3(64), (size_t)window * sizeof(float), stream, qkv, kcache,
                       vcache, out, rows, n, H, window, ring);
    CSM_CHECK_LAUNCH("csm_attn_window_stream_rows_f32");
    return 0;
}

extern "C" int csm_transpose_rows_f32(const float* in, float* out, int batch, int R, int C, hipStream_t stream) {
    CSM_REQUIRE(in && out && batch > 0 && batch <= 65535 && R > 0 && C > 0, "csm_transpose_rows_f32: bad arguments");
    CSM_REQUIRE((R + 31) / 32 <= 65535, "csm_transpose_rows_f32: %d rows exceed the grid (65535 * 32)", R);
    hipLaunchKernelGGL(transpose_f32_kernel, dim3((C + 31) / 32, (R + 31) / 32, batch), dim3(256), 0, stream, in, out, R, C);
    CSM_CHECK_LAUNCH("csm_transpose_rows_f32");
    return 0;
}

extern "C" int csm_conv1d_f32(const float* x, const float* w, const float* bias, const float* residual, float* y, int C_in,
                              int C_out, int T_in, int T_out, int k, int stride, int dilation, int pad_left, int pad_mode,
                              int groups, int elu_in, hipStream_t stream) {
    CSM_REQUIRE(x && w && y && C_in > 0 && C_out > 0 && T_in > 0 && T_out > 0 && k > 0 && stride > 0 && dilation > 0 && groups > 0 &&
                    C_in % groups == 0 && C_out % groups == 0 && C_out <= 65535, "csm_conv1d_f32: bad arguments");
    int bx = (T_out + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(conv1d_kernel, dim3(bx, C_out), dim3(256), 0, stream, x, w, bias, residual, y, C_in, C_out, T_in, T_out, k,
                       stride, dilation, pad_left, pad_mode, groups, elu_in);
    CSM_CHECK_LAUNCH("csm_conv1d_f32");
    return 0;
}

extern "C" int csm_conv_transpose1d_f32(const float* x, const float* w, const float* bias, float* y, int C_in, int C_out, int T_in,
                                        int T_out, int k, int stride, int crop_left, int groups, int elu_in, hipStream_t stream) {
    CSM_REQUIRE(x && w && y && C_in > 0 && C_out > 0 && T_in > 0 && T_out > 0 && k > 0 && stride > 0 && groups > 0 &&
                    C_in % groups == 0 && C_out % groups == 0 && C_out <= 65535, "csm_conv_transpose1d_f32: bad arguments");
    int bx = (T_out + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(conv_transpose1d_kernel, dim3(bx, C_out), dim3(256), 0, stream, x, w, bias, y, C_in, C_out, T_in, T_out, k,
                       stride, crop_left, groups, elu_in);
    CSM_CHECK_LAUNCH("csm_conv_transpose1d_f32");
    return 0;
}

extern "C" int csm_layernorm_f32(const float* x, const float* w, const float* b, float* y, int T, int D, float eps, hipStream_t stream) {
    CSM_REQUIRE(x && w && b && y && T > 0 && D > 0, "csm_layernorm_f32: bad arguments");
    hipLaunchKernelGGL(layernorm_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, x, w, b, y, T, D, eps);
    CSM_CHECK_LAUNCH("csm_layernorm_f32");
    return 0;
}

extern "C" int csm_linear_f32(const float* x, const float* W, const float* scale, const float* residual, float* y, int T, int N,
                              int K, int ldx, int act, hipStream_t stream) {
    CSM_REQUIRE(x && W && y && T > 0 && N > 0 && K > 0 && ldx >= K && (!scale || residual), "csm_linear_f32: bad arguments");
    if (T <= 16 && K % 32 == 0 && ((uintptr_t)W & 15) == 0)        // a few rows: one thread per output (same bits)
        hipLaunchKernelGGL(linear_f32_rows_kernel<8>, dim3((N + 255) / 256, T), dim3(256), 0, stream, x, W, scale, residual, y, T, N,
                           K, ldx, act);
    else
        hipLaunchKernelGGL(linear_f32_kernel, dim3((N + 63) / 64, (T + 63) / 64), dim3(256), 0, stream, x, W, scale, residual, y, T, N,
                           K, ldx, act);
    CSM_CHECK_LAUNCH("csm_linear_f32");
    return 0;
}

extern "C" int csm_rope_half_f32(float* qkv, int T, int H, int head_dim, float base, int pos0, hipStream_t stream) {
    CSM_REQUIRE(qkv && T > 0 && H > 0 && head_dim > 0 && (head_dim & 1) == 0, "csm_rope_half_f32: bad arguments");
    const long long total = (long long)T * 2 * H * (head_dim / 2);
    long long b = (total + 255) / 256;
    hipLaunchKernelGGL(rope_half_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, stream, qkv, T, H, head_dim, base, pos0);
    CSM_CHECK_LAUNCH("csm_rope_half_f32");
    return 0;
}

extern "C" int csm_attn_window_f32(const float* qkv, float* out, int T, int H, int head_dim, int window, hipStream_t stream) {
    CSM_REQUIRE(qkv && out && T > 0 && H > 0 && H <= 65535 && window > 0 && window <= 8192, "csm_attn_window_f32: bad arguments");
    CSM_REQUIRE(head_dim == 64, "csm_attn_window_f32: head_dim %d unsupported (64)", head_dim);
    hipLaunchKernelGGL((attn_f32_kernel<64>), dim3(T, H), dim3(64), (size_t)window * sizeof(float), stream, qkv, out, T, H, window);
    CSM_CHECK_LAUNCH("csm_attn_window_f32");
    return 0;
}

extern "C" int csm_conv1d_stream_f32(const float* hist, const float* x, const float* w, const float* bias, const float* residual,
                                     float* y, float* hist_out, int C_in, int C_out, int n, int k, int dilation, int groups, int elu_in,
                                     hipStream_t stream) {
    CSM_REQUIRE(x && w && y && C_in > 0 && C_out > 0 && n > 0 && k > 0 && dilation > 0 && groups > 0 && C_in % groups == 0 &&
                    C_out % groups == 0 && C_out <= 65535, "csm_conv1d_stream_f32: bad arguments");
    CSM_REQUIRE(k == 1 || (hist && hist_out && hist != hist_out), "csm_conv1d_stream_f32: k > 1 needs two distinct history buffers");
    int bx = (n + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(conv1d_stream_kernel, dim3(bx, C_out), dim3(256), 0, stream, hist, x, w, bias, residual, y, hist_out, C_in, C_out,
                       n, k, dilation, groups, elu_in);
    CSM_CHECK_LAUNCH("csm_conv1d_stream_f32");
    return 0;
}

extern "C" int csm_conv1d_stream_strided_f32(const float* hist, const float* x, const float* w, const float* bias, const float* residual,
                                             float* y, float* hist_out, int C_in, int C_out, int n_in, int k, int stride, int dilation,
                                             int groups, int elu_in, int edge_first, hipStream_t stream) {
    CSM_REQUIRE(x && w && y && C_in > 0 && C_out > 0 && n_in > 0 && k > 0 && stride > 0 && dilation > 0 && groups > 0 &&
                    C_in % groups == 0 && C_out % groups == 0 && C_out <= 65535, "csm_conv1d_stream_strided_f32: bad arguments");
    CSM_REQUIRE(n_in % stride == 0, "csm_conv1d_stream_strided_f32: n_in %d is not a multiple of stride %d", n_in, stride);
    const long long H = (long long)(k - 1) * dilation + 1 - stride;
    CSM_REQUIRE(H >= 0, "csm_conv1d_stream_strided_f32: stride %d exceeds the kernel's extent (k %d, dilation %d)", stride, k, dilation);
    CSM_REQUIRE(H + n_in < (1LL << 31), "csm_conv1d_stream_strided_f32: column index overflow");
    CSM_REQUIRE(H == 0 || (hist_out && hist != hist_out && (hist || edge_first)),
                "csm_conv1d_stream_strided_f32: a history of %lld columns needs two distinct history buffers", H);
    const int n_out = n_in / stride;
    const long long work = n_out > H ? n_out : H;              // the same grid writes the outputs and the next history
    const int bs = rows_block(work);
    long long bx = (work + bs - 1) / bs;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(conv1d_stream_strided_kernel, dim3((unsigned)bx, C_out), dim3(bs), 0, stream, hist, x, w, bias, residual, y,
                       hist_out, C_in, C_out, n_in, k, stride, dilation, groups, elu_in, edge_first ? 1 : 0);
    CSM_CHECK_LAUNCH("csm_conv1d_stream_strided_f32");
    return 0;
}

extern "C" int csm_conv_transpose1d_stream_f32(const float* hist, const float* x, const float* w, const float* bias, float* y,
                                               float* hist_out, int C_in, int C_out, int n, int pos0, int k, int stride, int groups,
                                               int elu_in, hipStream_t stream) {
    CSM_REQUIRE(x && w && y && C_in > 0 && C_out > 0 && n > 0 && pos0 >= 0 && k > 0 && stride > 0 && groups > 0 &&
                    C_in % groups == 0 && C_out % groups == 0 && C_out <= 65535 && (long long)(pos0 + (long long)n) * stride < (1LL << 31),
                "csm_conv_transpose1d_stream_f32: bad arguments");
    CSM_REQUIRE(k <= stride || (hist && hist_out && hist != hist_out),
                "csm_conv_transpose1d_stream_f32: k > stride needs two distinct history buffers");
    int bx = (n * stride + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(conv_transpose1d_stream_kernel, dim3(bx, C_out), dim3(256), 0, stream, hist, x, w, bias, y, hist_out, C_in, C_out,
                       n, pos0, k, stride, groups, elu_in);
    CSM_CHECK_LAUNCH("csm_conv_transpose1d_stream_f32");
    return 0;
}

extern "C" int csm_attn_window_stream_f32(const float* qkv, float* kcache, float* vcache, float* out, int n, int pos0, int H,
                                          int head_dim, int window, int ring, hipStream_t stream) {
    CSM_REQUIRE(qkv && kcache && vcache && out && n > 0 && pos0 >= 0 && H > 0 && H <= 65535 && window > 0 && window <= 8192 && n <= 65535,
                "csm_attn_window_stream_f32: bad arguments");
    CSM_REQUIRE(ring >= window + n - 1, "csm_attn_window_stream_f32: ring %d < window %d + n %d - 1", ring, window, n);
    CSM_REQUIRE(head_dim == 64, "csm_attn_window_stream_f32: head_dim %d unsupported (64)", head_dim);
    hipLaunchKernelGGL((attn_f32_stream_kernel<64>), dim3(n, H), dim3(64), (size_t)window * sizeof(float), stream, qkv, kcache, vcache, out,
                       pos0, H, window, ring);
    CSM_CHECK_LAUNCH("csm_attn_window_stream_f32");
    return 0;
}

extern "C" int csm_transpose_f32(const float* in, float* out, int R, int C, hipStream_t stream) {
    CSM_REQUIRE(in && out && R > 0 && C > 0, "csm_transpose_f32: bad arguments");
    CSM_REQUIRE((R + 31) / 32 <= 65535, "csm_transpose_f32: %d rows exceed the grid (65535 * 32)", R);
    hipLaunchKernelGGL(transpose_f32_kernel, dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, stream, in, out, R, C);
    CSM_CHECK_LAUNCH("csm_transpose_f32");
    return 0;
}
