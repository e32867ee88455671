// hulc_amd/csrc/aux_rows.h — the CLIP and MIA auxiliary losses on MORE than 64 flagged rows, and the routers that pick between them and the single-workgroup
// kernels (kernels.h clip_loss_kernel / clip_loss_wide_kernel, aux_heads.h mia_head_kernel), which keep n <= 64 exactly as it was.
//   clip_rows_stats_kernel / clip_rows_grad_kernel / clip_rows_finish_kernel   one workgroup per 64-row block, logits recomputed from LDS tiles, never stored
//   mia_rows_kernel / mia_rows_finish_kernel                                   one workgroup per 64 scored pairs, per-workgroup gradient slabs summed in a fixed order
// fp32 arithmetic in every engine; no float atomics: two runs give the same bits.
#pragma once
#include "aux_heads.h"
#include "kernels.h"

namespace HULC_NS {

constexpr int AUX_ROWS_SINGLE = 64;      // up to here one workgroup does the whole loss (the kernels this file does not touch)
constexpr int CLIP_TB = 64;              // rows of a block
constexpr int CLIP_D = 32;               // projection width
constexpr int CLIP_LD = CLIP_D + 1;

// floats of workspace the tiled CLIP kernels need for n rows: normalised img | normalised txt | |img| | |txt| | row max | row log-sum | column max | column log-sum |
// loss partials | d logit_scale partials.  A log-sum-exp is kept as its two parts (max, log of the scaled sum): at logit_scale = ln 100 their sum would be rounded
// at magnitude 100 (4e-6), an error that exp(L - lse) turns into a relative error of every g_ij of the row; (L - max) - log-sum has none of it.
inline int64_t clip_rows_ws_floats(int64_t n) { const int64_t nb = (n + CLIP_TB - 1) / CLIP_TB; return 2 * n * CLIP_D + 6 * n + 2 * nb; }
struct ClipRowsWs {
    float *in_n, *tn_n, *ni, *nt, *rowm, *rowls, *colm, *colls, *partl, *parts;
    __host__ __device__ ClipRowsWs(float* ws, int n) {
        const int nb = (n + CLIP_TB - 1) / CLIP_TB;
        in_n = ws; tn_n = in_n + (long long)n * CLIP_D; ni = tn_n + (long long)n * CLIP_D; nt = ni + n; rowm = nt + n; rowls = rowm + n; colm = rowls + n; colls = colm + n; partl = colls + n; parts = partl + nb;
    }
};

// s * <a, b> over the 32 elements in index order: the ONE form of a logit, so every pass that recomputes L_ij gets the same bits
DEVI float clip_logit(const float (&a)[CLIP_D], const float* __restrict__ b, float s) {
    float c = 0.f;
#pragma unroll
    for (int d = 0; d < CLIP_D; ++d) c = fmaf(a[d], b[d], c);
    return s * c;
}
// rows [r0, r0 + 64) of src (n, 32), L2-normalised, into an LDS tile; rows >= n read as zeros with norm 1; norm may be null.  256 threads: thread t owns 8 elements of row t / 4.
DEVI void clip_load_norm_tile(const float* __restrict__ src, int r0, int n, float (*tile)[CLIP_LD], float* norm) {
    const int t = threadIdx.x, r = t >> 2, d0 = (t & 3) * 8, gr = r0 + r;
    float v[8], a = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = gr < n ? src[(long long)gr * CLIP_D + d0 + k] : 0.f; a = fmaf(v[k], v[k], a); }
    a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64);
    const float nr = gr < n ? sqrtf(a) : 1.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[r][d0 + k] = v[k] / nr;
    if (norm && (t & 3) == 0) norm[r] = nr;
}
// the same rows, already normalised (workspace of the stats launch)
DEVI void clip_copy_tile(const float* __restrict__ src, int r0, int n, float (*tile)[CLIP_LD]) {
    const int t = threadIdx.x, r = t >> 2, d0 = (t & 3) * 8, gr = r0 + r;
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[r][d0 + k] = gr < n ? src[(long long)gr * CLIP_D + d0 + k] : 0.f;
}
// running log-sum-exp of one more logit
DEVI void lse_push(float& m, float& se, float l) {
    if (l > m) { se = se * expf(m - l) + 1.f; m = l; }
    else se += expf(l - m);
}

// Launch 1, workgroup b: the normalised rows and norms of its block (kept for launch 2), the log-sum-exp (as max and log-sum) of its img rows over ALL txt rows and of its txt rows over
// ALL img rows (it walks the blocks), and its share of the loss  sum_i (rowlse_i - L_ii) + (collse_i - L_ii), lse = max + log-sum.
// Thread t: row (or column) t % 64 of the own block against the 16 rows [16 (t / 64), +16) of the walked tile.
__global__ void __launch_bounds__(256) clip_rows_stats_kernel(const float* __restrict__ img, const float* __restrict__ txt, int n, const float* __restrict__ logit_scale,
                                                              float* __restrict__ ws) {
    __shared__ float oi[CLIP_TB][CLIP_LD], ot[CLIP_TB][CLIP_LD], wi[CLIP_TB][CLIP_LD], wt[CLIP_TB][CLIP_LD];
    __shared__ float noi[CLIP_TB], not_[CLIP_TB], mq[2][4][CLIP_TB], sq[2][4][CLIP_TB], red[CLIP_TB];
    const ClipRowsWs W(ws, n);
    const int t = threadIdx.x, r = t & 63, q = t >> 6, b = blockIdx.x, r0 = b * CLIP_TB, nb = gridDim.x;
    const float s = __expf(logit_scale[0]);
    clip_load_norm_tile(img, r0, n, oi, noi);
    clip_load_norm_tile(txt, r0, n, ot, not_);
    __syncthreads();
    {   // keep them for launch 2
        const int rr = t >> 2, d0 = (t & 3) * 8, gr = r0 + rr;
        if (gr < n) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { W.in_n[(long long)gr * CLIP_D + d0 + k] = oi[rr][d0 + k]; W.tn_n[(long long)gr * CLIP_D + d0 + k] = ot[rr][d0 + k]; }
            if ((t & 3) == 0) { W.ni[gr] = noi[rr]; W.nt[gr] = not_[rr]; }
        }
    }
    float a_i[CLIP_D], a_t[CLIP_D];
#pragma unroll
    for (int d = 0; d < CLIP_D; ++d) { a_i[d] = oi[r][d]; a_t[d] = ot[r][d]; }
    float mr = -INFINITY, sr = 0.f, mc = -INFINITY, sc = 0.f;
    for (int kb = 0; kb < nb; ++kb) {
        const int k0 = kb * CLIP_TB;
        __syncthreads();
        clip_load_norm_tile(img, k0, n, wi, nullptr);          // normalised again here: the walked block's workgroup may not have written its copy yet
        clip_load_norm_tile(txt, k0, n, wt, nullptr);
        __syncthreads();
        for (int jj = 0; jj < 16; ++jj) {
            const int j = q * 16 + jj;
            if (k0 + j < n) {
                lse_push(mr, sr, clip_logit(a_i, wt[j], s));      // L[r0 + r][k0 + j]
                lse_push(mc, sc, clip_logit(a_t, wi[j], s));      // L[k0 + j][r0 + r]: the same products in the same order as the row pass of block kb
            }
        }
    }
    mq[0][q][r] = mr; sq[0][q][r] = sr; mq[1][q][r] = mc; sq[1][q][r] = sc;
    __syncthreads();
    float part = 0.f;
    if (t < CLIP_TB && r0 + r < n) {
        float mx[2], ls[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float m = fmaxf(fmaxf(mq[h][0][r], mq[h][1][r]), fmaxf(mq[h][2][r], mq[h][3][r])), se = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) se += sq[h][k][r] > 0.f ? sq[h][k][r] * expf(mq[h][k][r] - m) : 0.f;
            mx[h] = m; ls[h] = logf(se);
        }
        W.rowm[r0 + r] = mx[0]; W.rowls[r0 + r] = ls[0]; W.colm[r0 + r] = mx[1]; W.colls[r0 + r] = ls[1];
        const float lii = clip_logit(a_i, ot[r], s);
        part = ((mx[0] - lii) + ls[0]) + ((mx[1] - lii) + ls[1]);
    }
    if (t < CLIP_TB) red[t] = part;
    __syncthreads();
    if (t == 0) {
        float acc = 0.f;
        for (int k = 0; k < CLIP_TB; ++k) acc += red[k];
        W.partl[b] = acc;
    }
}

// Launch 2, workgroup b: g_ij = (exp(L_ij - rowlse_i) + exp(L_ij - collse_j) - 2 delta_ij) / (2n) recomputed tile by tile; dimg of its img rows, dtxt of its txt
// rows (projection onto the tangent of the normalised vector, / norm, x w x lscale, as clip_loss_kernel) and its share of d logit_scale.
__global__ void __launch_bounds__(256) clip_rows_grad_kernel(int n, const float* __restrict__ logit_scale, float w, float* __restrict__ ws, float* __restrict__ dimg,
                                                             float* __restrict__ dtxt, const float* __restrict__ lscale) {
    if (lscale) w *= lscale[0];
    __shared__ float oi[CLIP_TB][CLIP_LD], ot[CLIP_TB][CLIP_LD], wi[CLIP_TB][CLIP_LD], wt[CLIP_TB][CLIP_LD], G[CLIP_TB][CLIP_TB + 1];
    __shared__ float wrm[CLIP_TB], wrs[CLIP_TB], wcm[CLIP_TB], wcs[CLIP_TB], red[4];
    const ClipRowsWs W(ws, n);
    const int t = threadIdx.x, r = t & 63, q = t >> 6, b = blockIdx.x, r0 = b * CLIP_TB, nb = gridDim.x;
    const int ar = t >> 2, ad0 = (t & 3) * 8;          // accumulation: 8 elements of row t / 4
    const float s = __expf(logit_scale[0]), inv2n = 1.f / (2.f * n);
    clip_copy_tile(W.in_n, r0, n, oi);
    clip_copy_tile(W.tn_n, r0, n, ot);
    __syncthreads();
    float a_i[CLIP_D], a_t[CLIP_D];
#pragma unroll
    for (int d = 0; d < CLIP_D; ++d) { a_i[d] = oi[r][d]; a_t[d] = ot[r][d]; }
    const bool own = r0 + r < n;
    const float orm = own ? W.rowm[r0 + r] : 0.f, ors = own ? W.rowls[r0 + r] : 0.f, ocm = own ? W.colm[r0 + r] : 0.f, ocs = own ? W.colls[r0 + r] : 0.f;
    float din[8], dtn[8], dsp = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { din[k] = 0.f; dtn[k] = 0.f; }
    for (int kb = 0; kb < nb; ++kb) {
        const int k0 = kb * CLIP_TB;
        __syncthreads();
        clip_copy_tile(W.in_n, k0, n, wi);
        clip_copy_tile(W.tn_n, k0, n, wt);
        if (t < CLIP_TB) {
            const bool in = k0 + t < n;
            wrm[t] = in ? W.rowm[k0 + t] : 0.f; wrs[t] = in ? W.rowls[k0 + t] : 0.f; wcm[t] = in ? W.colm[k0 + t] : 0.f; wcs[t] = in ? W.colls[k0 + t] : 0.f;
        }
        __syncthreads();
        // own img rows x the tile's txt rows
        for (int jj = 0; jj < 16; ++jj) {
            const int j = q * 16 + jj;
            float g = 0.f;
            if (own && k0 + j < n) {
                const float l = clip_logit(a_i, wt[j], s), dl = (r0 + r == k0 + j) ? 1.f : 0.f;
                g = ((expf((l - orm) - ors) - dl) + (expf((l - wcm[j]) - wcs[j]) - dl)) * inv2n;
                dsp += g * (l / s);
            }
            G[r][j] = g;
        }
        __syncthreads();
        for (int j = 0; j < CLIP_TB; ++j) {
            const float g = G[ar][j];
#pragma unroll
            for (int k = 0; k < 8; ++k) din[k] = fmaf(g, wt[j][ad0 + k], din[k]);
        }
        __syncthreads();
        // the tile's img rows x own txt rows, stored by own row
        for (int jj = 0; jj < 16; ++jj) {
            const int i = q * 16 + jj;
            float g = 0.f;
            if (own && k0 + i < n) {
                const float l = clip_logit(a_t, wi[i], s), dl = (r0 + r == k0 + i) ? 1.f : 0.f;
                g = ((expf((l - wrm[i]) - wrs[i]) - dl) + (expf((l - ocm) - ocs) - dl)) * inv2n;
            }
            G[r][i] = g;
        }
        __syncthreads();
        for (int i = 0; i < CLIP_TB; ++i) {
            const float g = G[ar][i];
#pragma unroll
            for (int k = 0; k < 8; ++k) dtn[k] = fmaf(g, wi[i][ad0 + k], dtn[k]);
        }
    }
    dsp = wave_sum(dsp);
    if ((t & 63) == 0) red[q] = dsp;
    float di = 0.f, dt = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { din[k] *= s; dtn[k] *= s; di = fmaf(oi[ar][ad0 + k], din[k], di); dt = fmaf(ot[ar][ad0 + k], dtn[k], dt); }
    di += __shfl_xor(di, 1, 64); di += __shfl_xor(di, 2, 64);
    dt += __shfl_xor(dt, 1, 64); dt += __shfl_xor(dt, 2, 64);
    const int gr = r0 + ar;
    if (gr < n) {
        const float ni = W.ni[gr], nt = W.nt[gr];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            dimg[(long long)gr * CLIP_D + ad0 + k] = w * (din[k] - oi[ar][ad0 + k] * di) / ni;
            dtxt[(long long)gr * CLIP_D + ad0 + k] = w * (dtn[k] - ot[ar][ad0 + k] * dt) / nt;
        }
    }
    __syncthreads();
    if (t == 0) W.parts[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Launch 3: the per-block partials in block order
__global__ void __launch_bounds__(64) clip_rows_finish_kernel(int n, int nb, const float* __restrict__ logit_scale, float w, const float* __restrict__ ws,
                                                              float* __restrict__ loss_out, float* __restrict__ dlogit_scale, int with_grad,
                                                              const float* __restrict__ lscale) {
    if (threadIdx.x) return;
    if (lscale) w *= lscale[0];
    const ClipRowsWs W(const_cast<float*>(ws), n);
    float l = 0.f, d = 0.f;
    for (int b = 0; b < nb; ++b) { l += W.partl[b]; if (with_grad) d += W.parts[b]; }
    loss_out[0] = l / (2.f * n);
    if (with_grad) dlogit_scale[0] += w * d * __expf(logit_scale[0]);
}

// The CLIP loss of n rows of 32-wide projections.  n <= 64: the single-workgroup kernels (`wide`: the 1024-thread form of the 16-bit engines).  Above: the three
// launches of this file; `ws` holds clip_rows_ws_floats(n) floats.  Above 64 rows a null dimg / dtxt / dlogit_scale means loss only (validation: the gradient launch
// is skipped); the single-workgroup kernels always write all three.
inline bool launch_clip_loss(hipStream_t st, bool wide, const float* img, const float* txt, int n, const float* logit_scale, float w, float* loss_out, float* dimg,
                             float* dtxt, float* dlogit_scale, const float* lscale, float* ws) {
    if (n < 1) return false;
    if (n <= AUX_ROWS_SINGLE) {
        if (!dimg || !dtxt || !dlogit_scale) return false;
        if (wide) hipLaunchKernelGGL(clip_loss_wide_kernel, dim3(1), dim3(1024), 0, st, img, txt, n, CLIP_D, logit_scale, w, loss_out, dimg, dtxt, dlogit_scale, lscale);
        else hipLaunchKernelGGL(clip_loss_kernel, dim3(1), dim3(64), 0, st, img, txt, n, CLIP_D, logit_scale, w, loss_out, dimg, dtxt, dlogit_scale, lscale);
        return true;
    }
    if (!ws) return false;
    const int nb = (n + CLIP_TB - 1) / CLIP_TB;
    const bool grad = dimg && dtxt && dlogit_scale;
    hipLaunchKernelGGL(clip_rows_stats_kernel, dim3(nb), dim3(256), 0, st, img, txt, n, logit_scale, ws);
    if (grad) hipLaunchKernelGGL(clip_rows_grad_kernel, dim3(nb), dim3(256), 0, st, n, logit_scale, w, ws, dimg, dtxt, lscale);
    hipLaunchKernelGGL(clip_rows_finish_kernel, dim3(1), dim3(64), 0, st, n, nb, logit_scale, w, (const float*)ws, loss_out, dlogit_scale, grad ? 1 : 0, lscale);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// MIA on n > 64 rows.  The 2n scored pairs are independent given img / txt: workgroup c scores the pairs [64 c, 64 c + 64) with the two sweeps of mia_head_kernel
// (W0 through LDS in chunks, hidden activations recomputed in the backward sweep).  Pair n + i reads txt[(i - 1) mod n] — over all n rows, wherever they sit.
// It writes, never adds: its loss / db1 partial, a slab [dW0 512x64 | db0 512 | dW1 512] and the input gradient of each of its pairs; mia_rows_finish_kernel sums
// the slabs in workgroup order into the gradient buffer and gives row i of dimg / dtxt its two pairs' shares.
constexpr int MIA_CP = 64;                                   // pairs of a workgroup
constexpr int MIA_SLAB = MIA_H * MIA_IN + 2 * MIA_H;         // floats of a workgroup's slab
inline int64_t mia_rows_ws_floats(int64_t n) { const int64_t nwg = (2 * n + MIA_CP - 1) / MIA_CP; return nwg * (MIA_SLAB + 2) + 2 * n * MIA_IN; }
struct MiaRowsWs {
    float *part, *slab, *dx;
    __host__ __device__ MiaRowsWs(float* ws, int n) { const int nwg = (2 * n + MIA_CP - 1) / MIA_CP; part = ws; slab = part + 2 * nwg; dx = slab + (long long)nwg * MIA_SLAB; }
};

__global__ void __launch_bounds__(1024) mia_rows_kernel(const float* __restrict__ img, const float* __restrict__ txt, int n, const float* __restrict__ W0,
                                                        const float* __restrict__ b0, const float* __restrict__ W1, const float* __restrict__ b1, float w,
                                                        float* __restrict__ ws, int backward, const float* __restrict__ lscale) {
    if (lscale) w *= lscale[0];
    constexpr int BUF = MIA_KC2 * MIA_WS + 2 * MIA_CP * MIA_HS;      // backward sweep: W chunk | dh | relu(h)
    static_assert(BUF >= MIA_KC1 * MIA_WS, "LDS carve");
    __shared__ __attribute__((aligned(16))) float xp[MIA_CP * MIA_IN];      // the pairs' input rows [img | txt]
    __shared__ __attribute__((aligned(16))) float buf[BUF];
    __shared__ float zs[MIA_CP], dzs[MIA_CP];
    const MiaRowsWs W(ws, n);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = 2 * n, p0 = blockIdx.x * MIA_CP, np = min(MIA_CP, P - p0);
    for (int i = tid; i < MIA_CP * MIA_IN; i += 1024) {
        const int lp = i >> 6, c = i & 63, p = p0 + lp;
        float v = 0.f;
        if (lp < np) {
            if (c < MIA_D) v = img[(long long)(p < n ? p : p - n) * MIA_D + c];
            else v = txt[(long long)(p < n ? p : (p - n + n - 1) % n) * MIA_D + c - MIA_D];
        }
        xp[i] = v;
    }
    // ---- forward sweep: z_p
    float acc[MIA_CP / 16];
#pragma unroll
    for (int j = 0; j < MIA_CP / 16; ++j) acc[j] = 0.f;
    for (int k0 = 0; k0 < MIA_H; k0 += MIA_KC1) {
        __syncthreads();
        for (int i = tid; i < MIA_KC1 * MIA_IN; i += 1024) buf[(i >> 6) * MIA_WS + (i & 63)] = W0[(long long)k0 * MIA_IN + i];
        __syncthreads();
        float4 wr[MIA_IN / 4];
#pragma unroll
        for (int q = 0; q < MIA_IN / 4; ++q) wr[q] = *reinterpret_cast<const float4*>(&buf[lane * MIA_WS + 4 * q]);
        const float bk = b0[k0 + lane], w1k = W1[k0 + lane];
#pragma unroll
        for (int j = 0; j < MIA_CP / 16; ++j) {
            const int lp = wave + 16 * j;
            if (lp < np) {
                const float4* x = reinterpret_cast<const float4*>(&xp[lp * MIA_IN]);
                float h = bk;
#pragma unroll
                for (int q = 0; q < MIA_IN / 4; ++q) { const float4 v = x[q]; h += wr[q].x * v.x; h += wr[q].y * v.y; h += wr[q].z * v.z; h += wr[q].w * v.w; }
                acc[j] += fmaxf(h, 0.f) * w1k;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MIA_CP / 16; ++j) {
        const int lp = wave + 16 * j;
        if (lp < np) { const float s = wave_sum(acc[j]); if (lane == 0) zs[lp] = s + b1[0]; }
    }
    __syncthreads();
    // ---- BCE with logits (stable form); the mean is over all 2n pairs
    const float gs = w / (float)P;
    if (tid < 64) {
        float l = 0.f, dz = 0.f;
        if (tid < np) {
            const float z = zs[tid], y = p0 + tid < n ? 1.f : 0.f;
            l = fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
            dz = (mia_sigmoid(z) - y) * gs;
        }
        dzs[tid] = dz;
        l = wave_sum(l); dz = wave_sum(dz);
        if (tid == 0) { W.part[2 * blockIdx.x] = l; W.part[2 * blockIdx.x + 1] = dz; }
    }
    if (!backward) return;

    // ---- backward sweep
    float* const slab = W.slab + (long long)blockIdx.x * MIA_SLAB;
    float* const Ws = buf;                                  // [KC2][WS]
    float* const dhs = buf + MIA_KC2 * MIA_WS;              // [CP][HS]: d loss / d (pre-activation)
    float* const hs = dhs + MIA_CP * MIA_HS;                // [CP][HS]: relu(h)
    float dxa[MIA_CP * MIA_IN / 1024];                      // d x_p[c] of the elements idx = tid + 1024 j (p = idx / 64, c = idx % 64)
#pragma unroll
    for (int j = 0; j < MIA_CP * MIA_IN / 1024; ++j) dxa[j] = 0.f;
    for (int k0 = 0; k0 < MIA_H; k0 += MIA_KC2) {
        __syncthreads();
        for (int i = tid; i < MIA_KC2 * MIA_IN; i += 1024) Ws[(i >> 6) * MIA_WS + (i & 63)] = W0[(long long)k0 * MIA_IN + i];
        __syncthreads();
        for (int idx = tid; idx < MIA_CP * MIA_KC2; idx += 1024) {
            const int kk = idx & (MIA_KC2 - 1), lp = idx / MIA_KC2;
            float hr = 0.f, dh = 0.f;
            if (lp < np) {
                const float4* wq = reinterpret_cast<const float4*>(&Ws[kk * MIA_WS]);
                const float4* x = reinterpret_cast<const float4*>(&xp[lp * MIA_IN]);
                float h = b0[k0 + kk];
#pragma unroll
                for (int q = 0; q < MIA_IN / 4; ++q) { const float4 v = x[q], ww = wq[q]; h += ww.x * v.x; h += ww.y * v.y; h += ww.z * v.z; h += ww.w * v.w; }
                hr = fmaxf(h, 0.f);
                dh = h > 0.f ? dzs[lp] * W1[k0 + kk] : 0.f;
            }
            hs[lp * MIA_HS + kk] = hr;
            dhs[lp * MIA_HS + kk] = dh;
        }
        __syncthreads();
        // dW0[k][c] = sum_p dh_p[k] x_p[c]: a thread owns column c of the rows kk and kk + 16
        {
            const int c = tid & 63, kk = tid >> 6;
            float s0 = 0.f, s1 = 0.f;
            for (int lp = 0; lp < np; ++lp) {
                const float x = xp[lp * MIA_IN + c];
                s0 += dhs[lp * MIA_HS + kk] * x; s1 += dhs[lp * MIA_HS + kk + 16] * x;
            }
            slab[(k0 + kk) * MIA_IN + c] = s0;
            slab[(k0 + kk + 16) * MIA_IN + c] = s1;
        }
        // db0[k] = sum_p dh_p[k] ; dW1[k] = sum_p dz_p relu(h_p[k])
        if (tid < MIA_KC2) {
            float s = 0.f;
            for (int lp = 0; lp < np; ++lp) s += dhs[lp * MIA_HS + tid];
            slab[MIA_H * MIA_IN + k0 + tid] = s;
        } else if (tid >= 64 && tid < 64 + MIA_KC2) {
            const int kk = tid - 64;
            float s = 0.f;
            for (int lp = 0; lp < np; ++lp) s += dzs[lp] * hs[lp * MIA_HS + kk];
            slab[MIA_H * MIA_IN + MIA_H + k0 + kk] = s;
        }
        // d x_p[c] += sum_k dh_p[k] W0[k][c]
#pragma unroll
        for (int j = 0; j < MIA_CP * MIA_IN / 1024; ++j) {
            const int idx = tid + 1024 * j, c = idx & 63, lp = idx >> 6;
            float s = 0.f;
#pragma unroll 8
            for (int kk = 0; kk < MIA_KC2; ++kk) s += dhs[lp * MIA_HS + kk] * Ws[kk * MIA_WS + c];
            dxa[j] += s;
        }
    }
#pragma unroll
    for (int j = 0; j < MIA_CP * MIA_IN / 1024; ++j) {
        const int idx = tid + 1024 * j;
        if ((idx >> 6) < np) W.dx[(long long)p0 * MIA_IN + idx] = dxa[j];
    }
}

// Sums what the nwg workgroups of mia_rows_kernel left, in workgroup order: loss_out[0] = mean BCE; with `backward` dW0 / db0 / dW1 / db1 += the slabs, and
// dimg / dtxt (n, 32) stored — or added to when `accum` — from the two pairs each row feeds: img_i pairs i and n + i, txt_j pair j and, rolled, pair n + (j + 1) mod n.
__global__ void __launch_bounds__(256) mia_rows_finish_kernel(int n, int nwg, const float* __restrict__ ws, float* __restrict__ loss_out, int backward,
                                                              float* __restrict__ dimg, float* __restrict__ dtxt, int accum, float* __restrict__ dW0,
                                                              float* __restrict__ db0, float* __restrict__ dW1, float* __restrict__ db1) {
    const MiaRowsWs W(const_cast<float*>(ws), n);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx == 0) {
        float l = 0.f, d = 0.f;
        for (int c = 0; c < nwg; ++c) { l += W.part[2 * c]; d += W.part[2 * c + 1]; }
        loss_out[0] = l / (float)(2 * n);
        if (backward) db1[0] += d;
    }
    if (!backward) return;
    if (idx < MIA_SLAB) {
        float s = 0.f;
        for (int c = 0; c < nwg; ++c) s += W.slab[(long long)c * MIA_SLAB + idx];
        float* o = idx < MIA_H * MIA_IN ? dW0 + idx : (idx < MIA_H * MIA_IN + MIA_H ? db0 + (idx - MIA_H * MIA_IN) : dW1 + (idx - MIA_H * MIA_IN - MIA_H));
        *o += s;
        return;
    }
    const long long e = idx - MIA_SLAB;
    if (e >= (long long)n * MIA_IN) return;
    const int i = (int)(e >> 6), c = (int)(e & 63);
    if (c < MIA_D) {
        const float v = W.dx[(long long)i * MIA_IN + c] + W.dx[(long long)(n + i) * MIA_IN + c];
        float* o = dimg + (long long)i * MIA_D + c;
        *o = accum ? *o + v : v;
    } else {
        const float v = W.dx[(long long)i * MIA_IN + c] + W.dx[(long long)(n + (i + 1) % n) * MIA_IN + c];
        float* o = dtxt + (long long)i * MIA_D + c - MIA_D;
        *o = accum ? *o + v : v;
    }
}

// The MIA head on n rows.  n <= 64: mia_head_kernel, one workgroup.  Above: the two launches of this file; `ws` holds mia_rows_ws_floats(n) floats.
// dW0 == nullptr: loss only (validation).
inline bool launch_mia_head(hipStream_t st, const float* img, const float* txt, int n, const float* W0, const float* b0, const float* W1, const float* b1, float w,
                            float* loss_out, float* dimg, float* dtxt, int accum, float* dW0, float* db0, float* dW1, float* db1, const float* lscale, float* ws) {
    if (n < 1) return false;
    if (n <= AUX_ROWS_SINGLE) {
        hipLaunchKernelGGL(mia_head_kernel, dim3(1), dim3(1024), 0, st, img, txt, n, W0, b0, W1, b1, w, loss_out, dimg, dtxt, accum, dW0, db0, dW1, db1, lscale);
        return true;
    }
    if (!ws) return false;
    const int nwg = (2 * n + MIA_CP - 1) / MIA_CP, backward = dW0 ? 1 : 0;
    if (backward && (!dimg || !dtxt || !db0 || !dW1 || !db1)) return false;
    hipLaunchKernelGGL(mia_rows_kernel, dim3(nwg), dim3(1024), 0, st, img, txt, n, W0, b0, W1, b1, w, ws, backward, lscale);
    const long long work = backward ? (long long)MIA_SLAB + (long long)n * MIA_IN : 1;
    hipLaunchKernelGGL(mia_rows_finish_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, n, nwg, (const float*)ws, loss_out, backward, dimg, dtxt, accum, dW0, db0,
                       dW1, db1);
    return true;
}

}  // namespace HULC_NS
