// hulc_amd/csrc/aux_heads.h — the two language auxiliary heads next to the CLIP loss (kernels.h clip_loss_kernel), on the gathered rows flagged by
// use_for_aux_lang_loss.  mia_head_kernel serves n <= 64 rows (MIA_MAXN); more rows go to the multi-workgroup kernels of aux_rows.h, which routes
// (launch_mia_head).  cosine_dist_loss_kernel strides its rows and serves any n:
//   mia_head_kernel          MIA cross-modality matching loss (hulc/models/hulc.py:606-648): the whole discriminator, forward and backward, one launch
//   cosine_dist_loss_kernel  BC-Z language regression loss (hulc.py:567-604): mean(1 - cos(pred, lang)) and its gradient
// fp32 arithmetic in every engine; single workgroup each (deterministic: fixed-order reductions, no atomics).
#pragma once
#include "common.h"

namespace HULC_NS {

constexpr int MIA_H = 512;        // hidden width of the discriminator (conf/model/mia_lang_discriminator/default.yaml)
constexpr int MIA_D = 32;         // width of each projection (proj_vis_lang output = latent goal features)
constexpr int MIA_IN = 2 * MIA_D;
constexpr int MIA_WS = 68;        // LDS row stride of a staged W0 row: 16-byte aligned rows for ds_read_b128
constexpr int MIA_KC1 = 64;       // hidden units staged per step of the forward sweep (one per lane)
constexpr int MIA_KC2 = 32;       // hidden units staged per step of the backward sweep
constexpr int MIA_HS = MIA_KC2 + 1;
constexpr int MIA_MAXN = 64;
constexpr int MIA_MAXP = 2 * MIA_MAXN;      // scored pairs: n matching + n rolled

DEVI float mia_sigmoid(float z) {
    if (z >= 0.f) return 1.f / (1.f + expf(-z));
    const float e = expf(z);
    return e / (1.f + e);
}

// Pair p < n scores [img_p | txt_p] with label 1, pair n + i scores [img_i | txt_{(i-1) mod n}] with label 0 (torch.roll(txt, 1, 0)).
//   z_p = W1 . relu(W0 x_p + b0) + b1 ;  loss = mean_p BCEWithLogits(z_p, y_p)  (unweighted, written to loss_out[0])
// Backward (skipped when dW0 == nullptr: validation), every gradient times w x lscale:
//   dimg / dtxt (n, 32): STORED, or ADDED to what the CLIP kernel left there when `accum` != 0;  dW0 (512,64), db0, dW1 (1,512), db1: added into the gradient buffer.
// One workgroup of 1024 threads.  W0 (128 KB) passes through LDS twice in chunks: a forward sweep for the logits (a wave owns pairs, a lane one hidden unit
// whose W0 row it holds in registers), then — the logits' gradients known — a backward sweep that recomputes the chunk's hidden activations instead of keeping
// all 2n x 512 of them.
__global__ void __launch_bounds__(1024) mia_head_kernel(const float* __restrict__ img, const float* __restrict__ txt, int n, const float* __restrict__ W0,
                                                        const float* __restrict__ b0, const float* __restrict__ W1, const float* __restrict__ b1, float w,
                                                        float* __restrict__ loss_out, float* __restrict__ dimg, float* __restrict__ dtxt, int accum,
                                                        float* __restrict__ dW0, float* __restrict__ db0, float* __restrict__ dW1, float* __restrict__ db1,
                                                        const float* __restrict__ lscale = nullptr) {
    if (n < 1 || n > MIA_MAXN) return;
    if (lscale) w *= lscale[0];
    constexpr int BUF = MIA_KC2 * MIA_WS + MIA_MAXP * MIA_HS + MIA_MAXP * MIA_HS;      // backward sweep: W chunk | dh | relu(h); >= KC1 * WS and >= MAXP * IN
    static_assert(BUF >= MIA_KC1 * MIA_WS && BUF >= MIA_MAXP * MIA_IN, "LDS carve");
    __shared__ __attribute__((aligned(16))) float xi[MIA_MAXN * MIA_D];
    __shared__ __attribute__((aligned(16))) float xt[MIA_MAXN * MIA_D];
    __shared__ __attribute__((aligned(16))) float buf[BUF];
    __shared__ float zs[MIA_MAXP], dzs[MIA_MAXP], red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = 2 * n;
    for (int i = tid; i < n * MIA_D; i += 1024) { xi[i] = img[i]; xt[i] = txt[i]; }
    // the two halves of pair p's input row
    auto irow = [&](int p) { return p < n ? p : p - n; };
    auto trow = [&](int p) { return p < n ? p : (p - n + n - 1) % n; };

    // ---- forward sweep: z_p
    float acc[MIA_MAXP / 16];
#pragma unroll
    for (int j = 0; j < MIA_MAXP / 16; ++j) acc[j] = 0.f;
    for (int k0 = 0; k0 < MIA_H; k0 += MIA_KC1) {
        __syncthreads();
        for (int i = tid; i < MIA_KC1 * MIA_IN; i += 1024) buf[(i >> 6) * MIA_WS + (i & 63)] = W0[(long long)k0 * MIA_IN + i];
        __syncthreads();
        float4 wr[MIA_IN / 4];
#pragma unroll
        for (int q = 0; q < MIA_IN / 4; ++q) wr[q] = *reinterpret_cast<const float4*>(&buf[lane * MIA_WS + 4 * q]);
        const float bk = b0[k0 + lane], w1k = W1[k0 + lane];
#pragma unroll
        for (int j = 0; j < MIA_MAXP / 16; ++j) {
            const int p = wave + 16 * j;
            if (p < P) {
                const float4* a = reinterpret_cast<const float4*>(&xi[irow(p) * MIA_D]);
                const float4* b = reinterpret_cast<const float4*>(&xt[trow(p) * MIA_D]);
                float h = bk;
#pragma unroll
                for (int q = 0; q < MIA_D / 4; ++q) { const float4 x = a[q]; h += wr[q].x * x.x; h += wr[q].y * x.y; h += wr[q].z * x.z; h += wr[q].w * x.w; }
#pragma unroll
                for (int q = 0; q < MIA_D / 4; ++q) { const float4 x = b[q]; const float4 ww = wr[MIA_D / 4 + q]; h += ww.x * x.x; h += ww.y * x.y; h += ww.z * x.z; h += ww.w * x.w; }
                acc[j] += fmaxf(h, 0.f) * w1k;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MIA_MAXP / 16; ++j) {
        const int p = wave + 16 * j;
        if (p < P) { const float s = wave_sum(acc[j]); if (lane == 0) zs[p] = s + b1[0]; }
    }
    __syncthreads();
    // ---- BCE with logits (stable form), mean over the 2n pairs; d loss / d z_p
    const float gs = w / (float)P;
    if (tid < 128) {
        float l = 0.f, dz = 0.f;
        if (tid < P) {
            const float z = zs[tid], y = tid < n ? 1.f : 0.f;
            l = fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
            dz = (mia_sigmoid(z) - y) * gs;
            dzs[tid] = dz;
        }
        l = wave_sum(l); dz = wave_sum(dz);
        if (lane == 0) { red[wave] = l; red[2 + wave] = dz; }
    }
    __syncthreads();
    if (tid == 0) {
        loss_out[0] = (red[0] + red[1]) / (float)P;
        if (db1) db1[0] += red[2] + red[3];
    }
    if (!dW0) return;

    // ---- backward sweep
    float* const Ws = buf;                                  // [KC2][WS]
    float* const dhs = buf + MIA_KC2 * MIA_WS;              // [P][HS]: d loss / d (pre-activation)
    float* const hs = dhs + MIA_MAXP * MIA_HS;              // [P][HS]: relu(h)
    float dxa[MIA_MAXP * MIA_IN / 1024];                    // d x_p[c] of the elements idx = tid + 1024 j (p = idx / 64, c = idx % 64)
#pragma unroll
    for (int j = 0; j < MIA_MAXP * MIA_IN / 1024; ++j) dxa[j] = 0.f;
    for (int k0 = 0; k0 < MIA_H; k0 += MIA_KC2) {
        __syncthreads();
        for (int i = tid; i < MIA_KC2 * MIA_IN; i += 1024) Ws[(i >> 6) * MIA_WS + (i & 63)] = W0[(long long)k0 * MIA_IN + i];
        __syncthreads();
        for (int idx = tid; idx < P * MIA_KC2; idx += 1024) {
            const int kk = idx & (MIA_KC2 - 1), p = idx / MIA_KC2;
            const float4* wq = reinterpret_cast<const float4*>(&Ws[kk * MIA_WS]);
            const float4* a = reinterpret_cast<const float4*>(&xi[irow(p) * MIA_D]);
            const float4* b = reinterpret_cast<const float4*>(&xt[trow(p) * MIA_D]);
            float h = b0[k0 + kk];
#pragma unroll
            for (int q = 0; q < MIA_D / 4; ++q) { const float4 x = a[q], ww = wq[q]; h += ww.x * x.x; h += ww.y * x.y; h += ww.z * x.z; h += ww.w * x.w; }
#pragma unroll
            for (int q = 0; q < MIA_D / 4; ++q) { const float4 x = b[q], ww = wq[MIA_D / 4 + q]; h += ww.x * x.x; h += ww.y * x.y; h += ww.z * x.z; h += ww.w * x.w; }
            hs[p * MIA_HS + kk] = fmaxf(h, 0.f);
            dhs[p * MIA_HS + kk] = h > 0.f ? dzs[p] * W1[k0 + kk] : 0.f;
        }
        __syncthreads();
        // dW0[k][c] = sum_p dh_p[k] x_p[c]: a thread owns column c of the rows kk and kk + 16
        {
            const int c = tid & 63, kk = tid >> 6;
            float s0 = 0.f, s1 = 0.f;
            for (int p = 0; p < P; ++p) {
                const float x = c < MIA_D ? xi[irow(p) * MIA_D + c] : xt[trow(p) * MIA_D + c - MIA_D];
                s0 += dhs[p * MIA_HS + kk] * x; s1 += dhs[p * MIA_HS + kk + 16] * x;
            }
            dW0[(long long)(k0 + kk) * MIA_IN + c] += s0;
            dW0[(long long)(k0 + kk + 16) * MIA_IN + c] += s1;
        }
        // db0[k] = sum_p dh_p[k] ; dW1[k] = sum_p dz_p relu(h_p[k])
        if (tid < MIA_KC2) {
            float s = 0.f;
            for (int p = 0; p < P; ++p) s += dhs[p * MIA_HS + tid];
            db0[k0 + tid] += s;
        } else if (tid >= 64 && tid < 64 + MIA_KC2) {
            const int kk = tid - 64;
            float s = 0.f;
            for (int p = 0; p < P; ++p) s += dzs[p] * hs[p * MIA_HS + kk];
            dW1[k0 + kk] += s;
        }
        // d x_p[c] += sum_k dh_p[k] W0[k][c]
#pragma unroll
        for (int j = 0; j < MIA_MAXP * MIA_IN / 1024; ++j) {
            const int idx = tid + 1024 * j, c = idx & 63, p = idx >> 6;
            if (p < P) {
                float s = 0.f;
#pragma unroll 8
                for (int kk = 0; kk < MIA_KC2; ++kk) s += dhs[p * MIA_HS + kk] * Ws[kk * MIA_WS + c];
                dxa[j] += s;
            }
        }
    }
    __syncthreads();
    float* const dxs = buf;                                 // [P][64]
#pragma unroll
    for (int j = 0; j < MIA_MAXP * MIA_IN / 1024; ++j) {
        const int idx = tid + 1024 * j;
        if ((idx >> 6) < P) dxs[idx] = dxa[j];
    }
    __syncthreads();
    // img_i feeds pairs i and n + i; txt_j feeds pair j and, rolled, pair n + (j + 1) mod n
    for (int idx = tid; idx < n * MIA_IN; idx += 1024) {
        const int i = idx >> 6, c = idx & 63;
        if (c < MIA_D) {
            const float v = dxs[i * MIA_IN + c] + dxs[(n + i) * MIA_IN + c];
            float* o = dimg + i * MIA_D + c;
            *o = accum ? *o + v : v;
        } else {
            const float v = dxs[i * MIA_IN + c] + dxs[(n + (i + 1) % n) * MIA_IN + c];
            float* o = dtxt + i * MIA_D + c - MIA_D;
            *o = accum ? *o + v : v;
        }
    }
}

// BC-Z: loss = mean_i (1 - p_i . t_i / (|p_i| |t_i|)) over n rows of D elements (plain quotient, no epsilon), written unweighted to loss_out[0];
// dpred_i = -(w x lscale / n) (t_i / (|p_i||t_i|) - (p_i . t_i) p_i / (|p_i|^3 |t_i|))  (skipped when dpred == nullptr).  One workgroup, one wave per row.
__global__ void __launch_bounds__(1024) cosine_dist_loss_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int n, int D, float w,
                                                                float* __restrict__ loss_out, float* __restrict__ dpred,
                                                                const float* __restrict__ lscale = nullptr) {
    if (lscale) w *= lscale[0];
    __shared__ float red[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float part = 0.f;
    for (int r = wave; r < n; r += 16) {
        const float* p = pred + (long long)r * D;
        const float* t = tgt + (long long)r * D;
        float pt = 0.f, pp = 0.f, tt = 0.f;
        for (int d = lane; d < D; d += 64) { const float a = p[d], b = t[d]; pt += a * b; pp += a * a; tt += b * b; }
        pt = wave_sum(pt); pp = wave_sum(pp); tt = wave_sum(tt);
        const float np = sqrtf(pp), nt = sqrtf(tt);
        part += 1.f - pt / (np * nt);
        if (dpred) {
            const float g = -w / (float)n, a = 1.f / (np * nt), b = pt / (np * np * np * nt);
            for (int d = lane; d < D; d += 64) dpred[(long long)r * D + d] = g * (t[d] * a - p[d] * b);
        }
    }
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < 16; ++i) s += red[i];
        loss_out[0] = s / (float)n;
    }
}

}  // namespace HULC_NS
