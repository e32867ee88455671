// hulc_amd/csrc/window_rows.h — the frame-store window tables (expand / compact) and the row kernels of the ragged encoder pass (expand / reduce) with their launchers:
// memory-bound index kernels of the engine's forward and ragged pass, no LDS.
#pragma once
#include "common.h"

namespace HULC_NS {

// variable-length windows (include/hulc_hip.h hulc_batch::window_len): window b holds L = clamp(wlen[b], 1, S) real frames starting at
// clamp(wstart[b], 0, nstore - L) and is padded to S by REPEATING its last real frame, store index and RandomShiftsAug shift both (the reference pads after the
// image transform: an exact duplicate).  The engine expands this ONCE per forward into a per-frame start table and the effective per-frame shifts; the conv1
// kernels then read the batch as a frame store of ONE-frame windows (Conv1Src: wstart = the table, S = 1) — the code they run is the fixed-window code, untouched.
__global__ void __launch_bounds__(256) window_expand_kernel(const long long* __restrict__ wstart, const int* __restrict__ wlen, int B, int S, long long nstore,
                                                            const int* __restrict__ sh_s, const int* __restrict__ sh_g, long long* __restrict__ frame_out,
                                                            int* __restrict__ sh_s_out, int* __restrict__ sh_g_out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * S) return;
    const int b = idx / S, t = idx - b * S;
    const int L = min(max(wlen[b], 1), (int)min((long long)S, nstore));      // a store shorter than S bounds L too: never an out-of-bounds read
    const long long s0 = min(max(wstart[b], 0ll), nstore - (long long)L);
    const int te = min(t, L - 1), fe = b * S + te;
    frame_out[idx] = s0 + te;
    if (sh_s) { sh_s_out[2 * idx] = sh_s[2 * fe]; sh_s_out[2 * idx + 1] = sh_s[2 * fe + 1]; }
    if (sh_g) { sh_g_out[2 * idx] = sh_g[2 * fe]; sh_g_out[2 * idx + 1] = sh_g[2 * fe + 1]; }
}
// ---- ragged encoder pass (include/hulc_hip.h hulc_batch::window_len_host): the encoders run on the REAL frames of the windows only.  lens[b] = L_b, already clamped
// on the host to [1, min(S, nstore)], off[b] = sum_{i<b} L_i (B + 1 entries), N' = off[B]: every index below derives from those two arrays, which the host built
// from ONE array, so a compact row is < N' by construction.  Three memory-bound row kernels, one thread per element or 16-byte piece, four full waves per block.
// The tables of window_expand_kernel without the duplicates: compact frame off[b] - off_base + t (t < L_b) is store frame s0 + t with shift row b * S + t.
// off_base: the paired pass's second batch has its own tables but shares the joint offsets (off_base = the first batch's N').
__global__ void __launch_bounds__(256) window_compact_kernel(const long long* __restrict__ wstart, const int* __restrict__ lens, const int* __restrict__ off, int off_base,
                                                             int B, int S, long long nstore, const int* __restrict__ sh_s, const int* __restrict__ sh_g,
                                                             long long* __restrict__ frame_out, int* __restrict__ sh_s_out, int* __restrict__ sh_g_out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * S) return;
    const int b = idx / S, t = idx - b * S, L = lens[b];
    if (t >= L) return;
    const long long s0 = min(max(wstart[b], 0ll), nstore - (long long)L);
    const int r = off[b] - off_base + t;
    frame_out[r] = s0 + t;
    if (sh_s) { sh_s_out[2 * r] = sh_s[2 * idx]; sh_s_out[2 * r + 1] = sh_s[2 * idx + 1]; }
    if (sh_g) { sh_g_out[2 * r] = sh_g[2 * idx]; sh_g_out[2 * r + 1] = sh_g[2 * idx + 1]; }
}
// dst [B*S][n] = src [N'][n] rows off[b] + min(t, L_b - 1): the padded rows are copies of the window's last real row.  16-byte pieces (n * sizeof(T) % 16 == 0)
template <typename T>
__global__ void __launch_bounds__(256) rows_expand_kernel(const T* __restrict__ src, const int* __restrict__ lens, const int* __restrict__ off, int B, int S, int n,
                                                          T* __restrict__ dst) {
    const int V = n * (int)sizeof(T) / 16;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * S * V) return;
    const int row = (int)(idx / V), v = (int)(idx - (long long)row * V), b = row / S, t = row - b * S;
    const long long r = off[b] + min(t, lens[b] - 1);
    reinterpret_cast<uint4*>(dst)[idx] = reinterpret_cast<const uint4*>(src)[r * V + v];
}
// dst [N'][n] fp32 from src [B*S][n] fp32: row off[b] + t = src[b, t] for t < L_b - 1, row off[b] + L_b - 1 = ((src[b, L_b-1] + src[b, L_b]) + ...) + src[b, S-1]:
// the gradients of a window's duplicates, summed in ascending t by ONE thread per float4 — a fixed order, no atomics.  Threads of the padded rows have nothing to do.
__global__ void __launch_bounds__(256) rows_reduce_kernel(const float* __restrict__ src, const int* __restrict__ lens, const int* __restrict__ off, int B, int S, int n,
                                                          float* __restrict__ dst) {
    const int V = n / 4;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * S * V) return;
    const int row = (int)(idx / V), v = (int)(idx - (long long)row * V), b = row / S, t = row - b * S, L = lens[b];
    if (t >= L) return;
    const float4* s = reinterpret_cast<const float4*>(src) + idx;
    float4 a = *s;
    if (t == L - 1)
        for (int u = t + 1; u < S; ++u) { const float4 x = s[(long long)(u - t) * V]; a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w; }
    reinterpret_cast<float4*>(dst)[(long long)(off[b] + t) * V + v] = a;
}
static inline void launch_window_compact(hipStream_t st, const long long* wstart, const int* lens, const int* off, int off_base, int B, int S, long long nstore,
                                         const int* sh_s, const int* sh_g, long long* frame_out, int* sh_s_out, int* sh_g_out) {
    hipLaunchKernelGGL(window_compact_kernel, dim3((B * S + 255) / 256), dim3(256), 0, st, wstart, lens, off, off_base, B, S, nstore, sh_s, sh_g, frame_out, sh_s_out, sh_g_out);
}
template <typename T> static inline void launch_rows_expand(hipStream_t st, const T* src, const int* lens, const int* off, int B, int S, int n, T* dst) {
    const long long pieces = (long long)B * S * (n * (int)sizeof(T) / 16);
    hipLaunchKernelGGL((rows_expand_kernel<T>), dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, src, lens, off, B, S, n, dst);
}
static inline void launch_rows_reduce(hipStream_t st, const float* src, const int* lens, const int* off, int B, int S, int n, float* dst) {
    const long long pieces = (long long)B * S * (n / 4);
    hipLaunchKernelGGL(rows_reduce_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, src, lens, off, B, S, n, dst);
}

}  // namespace HULC_NS
