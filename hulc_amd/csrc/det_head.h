// hulc_amd/csrc/det_head.h — the deterministic action decoder's head (hulc/models/decoders/deterministic_decoder.py): Linear(2048, 7) + tanh on the decoder's
// last hidden states, nn.HuberLoss / nn.MSELoss (reduction "mean"), and the head's three gradients.  Seven output columns are 7/16 of the narrowest GEMM tile,
// and every kernel here is bound by the bytes of H1 / dH1 it moves (4 KB per row in 16 bit), so none of them uses the matrix cores: 16-byte accesses, fp32
// accumulation, the 28 KB weight read through L1 / L2.
//   det_head_loss_kernel   forward + loss + gradient of the pre-activation, one wave per row
//   det_head_dgrad_kernel  dH1 = dpre W, and dZ1 = dH1 (H1 > 0) for the rows of the last time step (the first step of the layer-1 BPTT)
//   det_head_wgrad_kernel  per-slab partials of dW / db (256 rows each), summed in slab order by det_head_wgrad_sum_kernel: no float atomics, same bits every run
//   det_head_act_kernel    inference: tanh head + tcp -> world, optionally the validation metrics
// Rows are time-major (r = t B + b) like every decoder buffer; actions / robot_obs / pred are (B, S, ·) like the batch.
#pragma once
#include "iengine.h"      // HULC_CRIT_* (include/hulc_hip.h)
#include "kernels.h"
#include "plan_ln_launch.h"      // cdiv

namespace HULC_NS {

static constexpr int DET_HID = 2048;         // action_decoder.rnn hidden_size
static constexpr int DET_OUT = 7;            // out_features
static constexpr int DET_LD = 8;             // row stride of dpre (the 8th column is zero)
static constexpr int DET_SLAB_ROWS = 256;    // rows of one weight-gradient slab
static constexpr int DET_SLAB_COLS = 64;     // hidden columns of one weight-gradient workgroup
static constexpr int DET_SLAB = DET_OUT * DET_HID + 64;      // floats of one slab: dW [7][2048], then db [7]

// world -> tcp frame of a relative action (gripper_control.py:16-36), the arithmetic of logistic_loss_kernel
DEVI void det_world_to_tcp(const float* __restrict__ act, const float* __restrict__ ro, float (&at)[7]) {
    float R[9], Rn[9];
    euler_xyz(ro[3], ro[4], ro[5], R);
    euler_xyz(ro[3] + act[3] * 0.01f, ro[4] + act[4] * 0.01f, ro[5] + act[5] * 0.01f, Rn);
#pragma unroll
    for (int i = 0; i < 3; ++i) at[i] = R[0 + i] * act[0] + R[3 + i] * act[1] + R[6 + i] * act[2];
    auto Mij = [&](int i, int j) { return Rn[0 + i] * R[0 + j] + Rn[3 + i] * R[3 + j] + Rn[6 + i] * R[6 + j]; };
    float o[3] = {atan2f(-Mij(1, 2), Mij(2, 2)), asinf(fminf(1.f, fmaxf(-1.f, Mij(0, 2)))), atan2f(-Mij(0, 1), Mij(0, 0))};
    const float PI = 3.14159265358979323846f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (o[i] < -PI) o[i] += 2.f * PI;
        if (o[i] > PI) o[i] -= 2.f * PI;
        at[3 + i] = o[i] * 100.f;
    }
    at[6] = act[6];
}
// tcp -> world frame (gripper_control.py:39-63), the arithmetic of logistic_sample_kernel
DEVI void det_tcp_to_world(const float (&a)[7], const float* __restrict__ ro, float (&w)[7]) {
    float R[9], Rr[9];
    euler_xyz(ro[3], ro[4], ro[5], R);
    euler_xyz(a[3] * 0.01f, a[4] * 0.01f, a[5] * 0.01f, Rr);
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = R[3 * i] * a[0] + R[3 * i + 1] * a[1] + R[3 * i + 2] * a[2];
    auto Mij = [&](int i, int j) { return R[3 * i] * Rr[3 * j] + R[3 * i + 1] * Rr[3 * j + 1] + R[3 * i + 2] * Rr[3 * j + 2]; };   // R * Rr^T
    float o[3] = {atan2f(-Mij(1, 2), Mij(2, 2)), asinf(fminf(1.f, fmaxf(-1.f, Mij(0, 2)))), atan2f(-Mij(0, 1), Mij(0, 0))};
    const float PI = 3.14159265358979323846f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] -= ro[3 + i];
        if (o[i] < -PI) o[i] += 2.f * PI;
        if (o[i] > PI) o[i] -= 2.f * PI;
        w[3 + i] = o[i] * 100.f;
    }
    w[6] = a[6];
}

// 8 contiguous elements stored with 16-byte accesses (p is 16-byte aligned)
DEVI void det_store8(h16_t* p, const h16_t (&v)[8]) { *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(v); }
DEVI void det_store8(float* p, const float (&v)[8]) {
    reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// the seven dot products of one 2048-long row against W [7][2048], one wave: lane l takes the 8-element groups l, l + 64, ...; every lane returns all seven sums
template <typename T>
DEVI void det_row_dots(const T* __restrict__ h, const T* __restrict__ W, int lane, float (&acc)[DET_OUT]) {
#pragma unroll
    for (int j = 0; j < DET_OUT; ++j) acc[j] = 0.f;
#pragma unroll
    for (int i = 0; i < DET_HID / 512; ++i) {
        const int k = (i * 64 + lane) * 8;
        T hv[8];
        load8<T>(h + k, hv);
        float hf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) hf[e] = to_f<T>(hv[e]);
#pragma unroll
        for (int j = 0; j < DET_OUT; ++j) {
            T wv[8];
            load8<T>(W + (long long)j * DET_HID + k, wv);
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s += hf[e] * to_f<T>(wv[e]);
            acc[j] += s;
        }
    }
#pragma unroll
    for (int j = 0; j < DET_OUT; ++j) acc[j] = wave_sum(acc[j]);
}

// One wave per time-major row r = t B + b, four rows per workgroup.
//   pre = H1[r] W^T + bias, p = tanh(pre); d = p - target, target = the world-frame action (frame 0: DeterministicDecoder.loss returns the criterion against the
//   UNTRANSFORMED actions, deterministic_decoder.py:91-94) or world_to_tcp_frame(action, robot_obs) (frame 1: loss_and_act);
//   Huber (delta 1): 0.5 d^2 for |d| <= 1, else |d| - 0.5; MSE: d^2;  row_loss[r ldl] = sum_j l_j / 7 (summed j = 0..6 in order; columns 1..ldl-1 are zeroed);
//   dpre[r][j] = grad_scale (x lscale[0]) l'(d) (1 - p^2) / 7, dpre[r][7] = 0;  pred[(b S + t)][0..7) = tcp_to_world_frame(p, robot_obs).
// 1 - p^2 is evaluated as 4 e / (1 + e)^2 with e = exp(-2 |pre|): no cancellation where the prediction saturates.
template <typename T>
__global__ void __launch_bounds__(256) det_head_loss_kernel(const T* __restrict__ H1, const T* __restrict__ W, const float* __restrict__ bias,
                                                            const float* __restrict__ actions /*[B][S][7]*/, const float* __restrict__ robot_obs /*[B][S][15]*/, int B, int S,
                                                            int criterion, int frame, float grad_scale, const float* __restrict__ lscale, float* __restrict__ row_loss,
                                                            int ldl, float* __restrict__ pred /*[B][S][7] or null*/, float* __restrict__ dpre /*[S B][8]*/) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= B * S) return;
    if (lscale) grad_scale *= lscale[0];       // dynamic loss scale (fp16 mode): the gradient only, the loss rows stay unscaled
    float acc[DET_OUT];
    det_row_dots<T>(H1 + (long long)r * DET_HID, W, lane, acc);
    const int t = r / B, b = r % B;
    const long long bs = (long long)b * S + t;
    const float* act = actions + bs * 7;
    const float* ro = robot_obs + bs * 15;
    float tgt[7], p[7];
    if (frame) det_world_to_tcp(act, ro, tgt);
    else {
#pragma unroll
        for (int j = 0; j < 7; ++j) tgt[j] = act[j];
    }
    float loss = 0.f, mine = 0.f;
#pragma unroll
    for (int j = 0; j < DET_OUT; ++j) {
        const float pre = acc[j] + bias[j];
        p[j] = tanhf(pre);
        const float e = expf(-2.f * fabsf(pre)), dt = 4.f * e / ((1.f + e) * (1.f + e));
        const float d = p[j] - tgt[j];
        float l, g;
        if (criterion == HULC_CRIT_MSE) { l = d * d; g = 2.f * d; }
        else if (fabsf(d) <= 1.f) { l = 0.5f * d * d; g = d; }
        else { l = fabsf(d) - 0.5f; g = d > 0.f ? 1.f : -1.f; }
        loss += l;
        if (lane == j) mine = grad_scale * g * dt * (1.f / 7.f);
    }
    if (lane < DET_LD) dpre[(long long)r * DET_LD + lane] = mine;
    if (lane < ldl) row_loss[(long long)r * ldl + lane] = lane == 0 ? loss * (1.f / 7.f) : 0.f;
    if (pred) {
        float w[7];
        det_tcp_to_world(p, ro, w);
        if (lane < 7) {
            float v = w[0];
#pragma unroll
            for (int j = 1; j < 7; ++j) v = lane == j ? w[j] : v;
            pred[bs * 7 + lane] = v;
        }
    }
}

// dH1[r][k] = sum_j dpre[r][j] W[j][k].  A workgroup takes 8 rows; thread i keeps the W columns 8 i .. 8 i + 7 of all seven rows in registers (56 floats) and
// stores 16 bytes (16 bit) per row.  Rows of the last time step (r >= r_last) also write dZ1_last[r - r_last] = dH1 (H1 > 0): the BPTT's first step.
template <typename T>
__global__ void __launch_bounds__(256) det_head_dgrad_kernel(const float* __restrict__ dpre, const T* __restrict__ W, const T* __restrict__ H1, int rows, int r_last,
                                                             T* __restrict__ dH1, T* __restrict__ dZ1_last) {
    const int k = threadIdx.x * 8;
    float w[DET_OUT][8];
#pragma unroll
    for (int j = 0; j < DET_OUT; ++j) {
        T wv[8];
        load8<T>(W + (long long)j * DET_HID + k, wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) w[j][e] = to_f<T>(wv[e]);
    }
    const int r0 = blockIdx.x * 8, r1 = min(rows, r0 + 8);
    for (int r = r0; r < r1; ++r) {
        const float4 d0 = *reinterpret_cast<const float4*>(dpre + (long long)r * DET_LD), d1 = *reinterpret_cast<const float4*>(dpre + (long long)r * DET_LD + 4);
        const float d[DET_OUT] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z};
        alignas(16) T o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < DET_OUT; ++j) s += d[j] * w[j][e];
            o[e] = from_f<T>(s);
        }
        det_store8(dH1 + (long long)r * DET_HID + k, o);
        if (r >= r_last) {
            T hv[8];
            load8<T>(H1 + (long long)r * DET_HID + k, hv);
            alignas(16) T z[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = to_f<T>(hv[e]) > 0.f ? o[e] : from_f<T>(0.f);
            det_store8(dZ1_last + (long long)(r - r_last) * DET_HID + k, z);
        }
    }
}

// Slab partials of dW[j][k] = sum_r dpre[r][j] H1[r][k] and db[j] = sum_r dpre[r][j].  grid (2048 / 64, ceil(rows / 256)): workgroup (x, z) owns the hidden columns
// 64 x .. 64 x + 63 of the rows 256 z .. 256 z + 255.  Thread (g = tid / 8, c = tid % 8) adds the rows g, g + 32, ... of the slab for its 8 columns (one 16-byte load
// per row in 16 bit); the 32 row groups are then summed through LDS in the order g = 0..31.  Every element of the slab is written (rows beyond `rows` add nothing).
template <typename T>
__global__ void __launch_bounds__(256) det_head_wgrad_kernel(const float* __restrict__ dpre, const T* __restrict__ H1, int rows, float* __restrict__ part) {
    __shared__ float red[32][DET_OUT * DET_SLAB_COLS + 8];
    const int tid = threadIdx.x, g = tid >> 3, c = tid & 7;
    const int k = blockIdx.x * DET_SLAB_COLS + c * 8;
    const int r0 = blockIdx.y * DET_SLAB_ROWS, r1 = min(rows, r0 + DET_SLAB_ROWS);
    float acc[DET_OUT][8], sb[DET_OUT];
#pragma unroll
    for (int j = 0; j < DET_OUT; ++j) {
        sb[j] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
    }
    for (int r = r0 + g; r < r1; r += 32) {
        const float4 d0 = *reinterpret_cast<const float4*>(dpre + (long long)r * DET_LD), d1 = *reinterpret_cast<const float4*>(dpre + (long long)r * DET_LD + 4);
        const float d[DET_OUT] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z};
        T hv[8];
        load8<T>(H1 + (long long)r * DET_HID + k, hv);
#pragma unroll
        for (int j = 0; j < DET_OUT; ++j) {
            sb[j] += d[j];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][e] += d[j] * to_f<T>(hv[e]);
        }
    }
#pragma unroll
    for (int j = 0; j < DET_OUT; ++j) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[g][j * DET_SLAB_COLS + c * 8 + e] = acc[j][e];
        if (c == 0) red[g][DET_OUT * DET_SLAB_COLS + j] = sb[j];
    }
    __syncthreads();
    float* slab = part + (long long)blockIdx.y * DET_SLAB;
    for (int o = tid; o < DET_OUT * DET_SLAB_COLS; o += 256) {
        float s = red[0][o];
        for (int q = 1; q < 32; ++q) s += red[q][o];
        const int j = o / DET_SLAB_COLS, kk = o % DET_SLAB_COLS;
        slab[(long long)j * DET_HID + blockIdx.x * DET_SLAB_COLS + kk] = s;
    }
    if (blockIdx.x == 0 && tid < DET_OUT) {
        float s = red[0][DET_OUT * DET_SLAB_COLS + tid];
        for (int q = 1; q < 32; ++q) s += red[q][DET_OUT * DET_SLAB_COLS + tid];
        slab[DET_OUT * DET_HID + tid] = s;
    }
}
// dW += the slabs in slab order, db likewise: the bound gradients ACCUMULATE (a second backward before the optimizer, the paired pass)
__global__ void __launch_bounds__(256) det_head_wgrad_sum_kernel(const float* __restrict__ part, int nslab, float* __restrict__ dW, float* __restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= DET_OUT * DET_HID + DET_OUT) return;
    float s = part[i];
    for (int z = 1; z < nslab; ++z) s += part[(long long)z * DET_SLAB + i];
    if (i < DET_OUT * DET_HID) dW[i] += s;
    else db[i - DET_OUT * DET_HID] += s;
}

// Inference: one wave per row, four rows per workgroup.  Row r of the call reads h1 + r 2048, or — rowdesc given (the batched rollout's slot state) — the NEW
// state of slot rowdesc[r]; robot_obs / pred / actions_gt are indexed (b S + t) for the time-major row r = t B + b (a rollout has S = 1).  metrics (validation):
// [0..5] += |err| / (B S), [6] += gripper sign match / (B S), the slots logistic_sample_kernel fills.
template <typename T>
__global__ void __launch_bounds__(256) det_head_act_kernel(const T* __restrict__ h1, const int* __restrict__ rowdesc, int max_envs, const T* __restrict__ W,
                                                           const float* __restrict__ bias, const float* __restrict__ robot_obs, const float* __restrict__ actions_gt, int B,
                                                           int S, float* __restrict__ pred, float* __restrict__ metrics) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= B * S) return;
    const T* h = h1 + (long long)r * DET_HID;
    if (rowdesc) { const int d = rowdesc[r]; h = h1 + ((long long)(1 - ((d >> 16) & 1)) * max_envs + (d & 0xffff)) * DET_HID; }
    float acc[DET_OUT];
    det_row_dots<T>(h, W, lane, acc);
    const int t = r / B, b = r % B;
    const long long bs = (long long)b * S + t;
    float p[7], w[7];
#pragma unroll
    for (int j = 0; j < DET_OUT; ++j) p[j] = tanhf(acc[j] + bias[j]);
    det_tcp_to_world(p, robot_obs + bs * 15, w);
    if (lane < 7) {
        float v = w[0];
#pragma unroll
        for (int j = 1; j < 7; ++j) v = lane == j ? w[j] : v;
        pred[bs * 7 + lane] = v;
        if (metrics && actions_gt) {
            const float inv = 1.f / (float)(B * S), gt = actions_gt[bs * 7 + lane];
            if (lane < 6) atomicAdd(metrics + lane, fabsf(v - gt) * inv);
            else atomicAdd(metrics + 6, (((v > 0.f) ? 1.f : -1.f) == gt) ? inv : 0.f);
        }
    }
}

// ---- launches (the engine and the test entries of k_entries.h go through these)
template <typename T>
inline void launch_det_head_loss(hipStream_t st, const T* H1, const T* W, const float* bias, const float* actions, const float* robot_obs, int B, int S, int criterion, int frame,
                                 float grad_scale, const float* lscale, float* row_loss, int ldl, float* pred, float* dpre) {
    hipLaunchKernelGGL((det_head_loss_kernel<T>), dim3(cdiv(B * S, 4)), dim3(256), 0, st, H1, W, bias, actions, robot_obs, B, S, criterion, frame, grad_scale, lscale, row_loss, ldl,
                       pred, dpre);
}
template <typename T>
inline void launch_det_head_dgrad(hipStream_t st, const float* dpre, const T* W, const T* H1, int B, int S, T* dH1, T* dZ1_last) {
    hipLaunchKernelGGL((det_head_dgrad_kernel<T>), dim3(cdiv(B * S, 8)), dim3(256), 0, st, dpre, W, H1, B * S, (S - 1) * B, dH1, dZ1_last);
}
static inline int det_head_slabs(int rows) { return cdiv(rows, DET_SLAB_ROWS); }
// part: det_head_slabs(rows) * DET_SLAB floats of scratch
template <typename T>
inline void launch_det_head_wgrad(hipStream_t st, const float* dpre, const T* H1, int rows, float* part, float* dW, float* db) {
    const int nz = det_head_slabs(rows);
    hipLaunchKernelGGL((det_head_wgrad_kernel<T>), dim3(DET_HID / DET_SLAB_COLS, nz), dim3(256), 0, st, dpre, H1, rows, part);
    hipLaunchKernelGGL(det_head_wgrad_sum_kernel, dim3(cdiv(DET_OUT * DET_HID + DET_OUT, 256)), dim3(256), 0, st, (const float*)part, nz, dW, db);
}
template <typename T>
inline void launch_det_head_act(hipStream_t st, const T* h1, const int* rowdesc, int max_envs, const T* W, const float* bias, const float* robot_obs, const float* actions_gt, int B,
                                int S, float* pred, float* metrics) {
    hipLaunchKernelGGL((det_head_act_kernel<T>), dim3(cdiv(B * S, 4)), dim3(256), 0, st, h1, rowdesc, max_envs, W, bias, robot_obs, actions_gt, B, S, pred, metrics);
}

}  // namespace HULC_NS
