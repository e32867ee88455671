// hulc_amd/csrc/rollout_step.h — the decoder step of the batched multi-environment rollout (hulc_rollout_envs_*, include/hulc_hip.h): N independent policy
// slots per context, n <= 64 of them stepped by one call.  From the encoder embedding to the (n,7) world-frame actions a 16-bit engine runs THREE launches:
//   env_rnn_layer_kernel (layer 0)  h0'[slot] = relu(emb_gripper[row] W_ih0[:, emb cols]^T + h0[slot] W_hh0^T + cache[slot])
//   env_rnn_layer_kernel (layer 1)  h1'[slot] = relu(h0'[slot] W_ih1^T + h1[slot] W_hh1^T + b_ih1 + b_hh1)
//   env_heads_sample_kernel         heads = h1'[slot] W_heads^T + b, logistic-mixture sample, gripper argmax, tcp -> world frame
// and no copy.  `cache` is the time-invariant decoder input term (plan embedding gather + goal W_ih0[:, goal cols]^T + b_ih0 + b_hh0), written per slot by
// env_plan_store_kernel when the slot is planned (or its state installed) — it only changes at a replan.
// The feed-forward body (hulc_decoder_body_select, rnn_model = mlp_decoder) runs the same kernels in their recurrence-free forms (REC = false), FOUR launches:
//   env_rnn_layer_kernel<false, true>   a0[row] = relu(emb_gripper[row] W_0[:, emb cols]^T + cache[slot])
//   env_rnn_layer_kernel<false, true>   a1[row] = relu(a0[row] W_1^T + b_1)
//   env_rnn_layer_kernel<false, false>  y[row]  = a1[row] W_2^T + b_2
//   env_heads_sample_kernel<NT, true>   heads = y[row] W_heads^T + b, ...
// a0 / a1 / y are ROW buffers [n][2048] of the call (the decoder's forward workspace): there is no per-slot hidden state, no parity, and `cache` holds one bias.
//
// State layout (device memory, owned by the engine; S = max_envs):
//   plan_i [S][32] int32 (hulc) / plan_f [S][256] fp32 (mcil) / goal [S][32] T / cache [S][2048] fp32 (16-bit engines) /
//   h0, h1 [2][S][2048] T: each layer's hidden state is DOUBLE-BUFFERED per slot.
// Every row of a call arrives as one descriptor word  slot | parity << 16  (rowdesc, copied to the device once per call): the slot's current state is
// h[parity][slot], the step writes h[1 - parity][slot].  The host flips a slot's parity after every act that named it, so the two buffers alternate PER
// SLOT: a slot that sits out a call keeps its parity and neither of its rows is touched; a slot's two layers always share one parity.
#pragma once
#include "common.h"

namespace HULC_NS {

static constexpr int ENV_HID = 2048;          // decoder hidden width (action_decoder.rnn hidden_size)
static constexpr int ENV_MAX_ROWS = 64;       // rows of one call: four 16-row MFMA tiles
static constexpr int ENV_COLS = 16;           // output columns of one workgroup of the layer kernel
static constexpr int ENV_WAVES = 8;

// 8 contiguous 16-bit elements as an MFMA fragment.  a16 (wave-uniform): the address is 16-byte aligned; otherwise two 8-byte loads — the weight matrices are views
// of the bound parameter layout, whose element offsets are only promised to be multiples of 4
DEVI h16x8_t env_ld8(const h16_t* p, bool a16) {
    union { h16x8_t v; uint2 u[2]; } x;
    if (a16) x.v = *reinterpret_cast<const h16x8_t*>(p);
    else { x.u[0] = *reinterpret_cast<const uint2*>(p); x.u[1] = *reinterpret_cast<const uint2*>(p + 4); }
    return x.v;
}
DEVI int env_slot(int desc) { return desc & 0xffff; }
DEVI int env_par(int desc) { return (desc >> 16) & 1; }

struct EnvLayerP {
    const int* rowdesc; int n, max_envs;
    const h16_t* x; long long x_ld; int x_by_slot, Kx;      // x_by_slot 0: row r of the call at x + r x_ld; 1: the NEW state of the layer below, x[(1 - parity) S + slot]
    const h16_t* Wx; long long wx_ld;                        // [2048][wx_ld], the first Kx columns of every row are used
    const h16_t* Whh;                                        // [2048][2048]; REC = false: unused
    h16_t* h;                                                // [2][S][2048] of this layer; REC = false: the output ROW buffer [n][2048]
    const float* ctab;                                       // [S][2048] per-slot constant (layer 0) or null
    const float *b1, *b2;                                    // ctab == null: c = b1 + b2 (REC = false: c = b1)
    int w16;                                                 // Wx and Whh rows are 16-byte aligned
};

// One recurrent layer for all rows of the call: out[r][c] = relu(sum_k x[r][k] Wx[c][k] + sum_k h[r][k] Whh[c][k] + c[r][c]).
// grid = 2048 / 16 workgroups, each owns 16 output columns for ALL rows, so every weight byte is read once per call (the 8 MB W_hh panel streams from HBM
// once; the <= 256 KB of h rows every workgroup reads stay in the L2 of its XCD).  The 8 waves split K (the x segment and the h segment, 32-wide steps, wave w
// takes steps w, w + 8, ...); a wave keeps one fp32 accumulator tile per 16-row tile across BOTH segments, the 8 partial tiles are summed through LDS in wave
// order (a fixed order: a row's result depends neither on its position in the call nor on its neighbours).  Operands are read straight from global memory
// into the MFMA fragments (A = 16 weight rows, B = 16 state rows: each lane's 8 k-elements are 16 contiguous bytes) — no LDS staging, no LDS-DMA.
// Why two buffers: every workgroup reads WHOLE h rows while the other 127 write their 16 columns of the new state; in place a late workgroup would read
// columns of step t + 1.  No grid barrier, no flags: the dependent layer is the next launch on the stream.
// REC = false (feed-forward body): no h segment, one bias, the output goes to row r of p.h (a row buffer no workgroup of this launch reads); RELU = false: the
// body's third layer.  <true, true> is the recurrent layer.
template <bool REC, bool RELU>
__global__ void __launch_bounds__(ENV_WAVES * 64) env_rnn_layer_kernel(EnvLayerP p) {
    __shared__ float4 red[ENV_WAVES][4][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, kq = (lane >> 4) * 8;
    const int c0 = blockIdx.x * ENV_COLS;
    const int ntile = (p.n + 15) >> 4;
    const h16_t* xr[4]; const h16_t* hr[4]; bool ok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = t * 16 + lr;
        ok[t] = r < p.n;
        const int d = ok[t] ? p.rowdesc[r] : 0;
        const long long cur = (long long)env_par(d) * p.max_envs + env_slot(d), nxt = (long long)(1 - env_par(d)) * p.max_envs + env_slot(d);
        hr[t] = REC ? p.h + cur * ENV_HID + kq : nullptr;
        xr[t] = (p.x_by_slot ? p.x + nxt * p.x_ld : p.x + (long long)r * p.x_ld) + kq;
    }
    const h16_t* wxr = p.Wx + (long long)(c0 + lr) * p.wx_ld + kq;
    const h16_t* whr = REC ? p.Whh + (long long)(c0 + lr) * ENV_HID + kq : nullptr;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const h16x8_t zero8v = {};
    // x segment
    const int nkx = p.Kx >> 5;
#pragma unroll 4
    for (int ks = wave; ks < nkx; ks += ENV_WAVES) {
        const h16x8_t wf = env_ld8(wxr + ks * 32, p.w16);
        h16x8_t xf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) xf[t] = (t < ntile && ok[t]) ? *reinterpret_cast<const h16x8_t*>(xr[t] + ks * 32) : zero8v;
#pragma unroll
        for (int t = 0; t < 4; ++t) if (t < ntile) acc[t] = MFMA_16x16x32_H(wf, xf[t], acc[t], 0, 0, 0);      // D^T: lane = state row, registers = 4 consecutive output columns
    }
    // h segment: 64 steps, 8 per wave
    if constexpr (REC) {
#pragma unroll 4
    for (int i = 0; i < ENV_HID / 32 / ENV_WAVES; ++i) {
        const int k = (wave + i * ENV_WAVES) * 32;
        const h16x8_t wf = env_ld8(whr + k, p.w16);
        h16x8_t xf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) xf[t] = (t < ntile && ok[t]) ? *reinterpret_cast<const h16x8_t*>(hr[t] + k) : zero8v;
#pragma unroll
        for (int t = 0; t < 4; ++t) if (t < ntile) acc[t] = MFMA_16x16x32_H(wf, xf[t], acc[t], 0, 0, 0);
    }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) if (t < ntile) red[wave][t][lane] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    __syncthreads();
    if (tid >= ntile * 64) return;
    const int t = tid >> 6, r = t * 16 + lr;
    if (r >= p.n) return;
    float4 s = red[0][t][lane];
#pragma unroll
    for (int w = 1; w < ENV_WAVES; ++w) { const float4 q = red[w][t][lane]; s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w; }
    const int d = p.rowdesc[r], slot = env_slot(d);
    const int c = c0 + (lane >> 4) * 4;
    float4 cc;
    if (p.ctab) cc = *reinterpret_cast<const float4*>(p.ctab + (long long)slot * ENV_HID + c);
    else if constexpr (REC) { const float4 a = *reinterpret_cast<const float4*>(p.b1 + c), b = *reinterpret_cast<const float4*>(p.b2 + c); cc = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
    else cc = *reinterpret_cast<const float4*>(p.b1 + c);
    s.x += cc.x; s.y += cc.y; s.z += cc.z; s.w += cc.w;
    if constexpr (RELU) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f); }
    uint2 o;
    o.x = pack2h(s.x, s.y);
    o.y = pack2h(s.z, s.w);
    const long long orow = REC ? (long long)(1 - env_par(d)) * p.max_envs + slot : (long long)r;
    *reinterpret_cast<uint2*>(p.h + orow * ENV_HID + c) = o;
}

DEVI void env_euler_xyz(float a, float b, float c, float (&R)[9]) {
    float sa, ca, sb, cb, sc, cc;
    sincosf(a, &sa, &ca); sincosf(b, &sb, &cb); sincosf(c, &sc, &cc);
    R[0] = cb * cc;                 R[1] = -cb * sc;                R[2] = sb;
    R[3] = ca * sc + sa * sb * cc;  R[4] = ca * cc - sa * sb * sc;  R[5] = -sa * cb;
    R[6] = sa * sc - ca * sb * cc;  R[7] = sa * cc + ca * sb * sc;  R[8] = ca * cb;
}

struct EnvHeadsP {
    const int* rowdesc; int n, max_envs;
    const h16_t* h1;                  // [2][S][2048]: the NEW layer-1 state h1[1 - parity][slot] is read; BYROW: [n][2048], row r of the call
    const h16_t* W;                   // packed heads [NHEAD][2048]: prob | mean | log_scale | gripper | zero pad
    const float* bias;                // [NHEAD]
    const float* robot_obs;           // [n][15]
    const float *u_mix, *u_act;       // [n][NDIM][NMIX] / [n][NDIM] injected uniform draws or null (counter RNG)
    int NMIX, NDIM; float log_scale_min; int gripper_control, discrete_gripper;
    unsigned long long seed;
    float* pred;                      // [n][7]
};

// Heads GEMM (K = 2048, NT * 16 packed head columns) + the sampler of logistic_sample_kernel (kernels.h; logistic_decoder_rnn.py:234-258) + the tcp -> world map
// (gripper_control.py:39-63) for one 16-row tile per workgroup: a workgroup owns COMPLETE rows of heads, so sampling needs no second pass.  The 8 waves split K
// (256 each, NT accumulator tiles per wave), the partial tiles are summed through LDS in two rounds (waves 4..7 into 0..3, then 0..3 in order): a fixed order again.
// BYROW (feed-forward body): the heads read row r of a row buffer, not a slot's state.
template <int NT, bool BYROW = false>
__global__ void __launch_bounds__(ENV_WAVES * 64) env_heads_sample_kernel(EnvHeadsP p) {
    __shared__ float4 red[4][NT][64];
    __shared__ float act_s[16][8];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, kq = (lane >> 4) * 8;
    const int r0 = blockIdx.x * 16;
    const bool ok = r0 + lr < p.n;
    const int d = ok ? p.rowdesc[r0 + lr] : 0;
    const h16_t* hrow = p.h1 + (BYROW ? (long long)(ok ? r0 + lr : 0) : (long long)(1 - env_par(d)) * p.max_envs + env_slot(d)) * ENV_HID + kq;
    const h16_t* wrow = p.W + (long long)lr * ENV_HID + kq;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const h16x8_t zero8v = {};
#pragma unroll 2
    for (int i = 0; i < ENV_HID / 32 / ENV_WAVES; ++i) {
        const int k = (wave * (ENV_HID / 32 / ENV_WAVES) + i) * 32;
        const h16x8_t hf = ok ? *reinterpret_cast<const h16x8_t*>(hrow + k) : zero8v;
        h16x8_t wf[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const h16x8_t*>(wrow + (long long)j * 16 * ENV_HID + k);
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = MFMA_16x16x32_H(wf[j], hf, acc[j], 0, 0, 0);       // D^T: lane & 15 = row of the tile, registers = head columns 16 j + 4 (lane >> 4) + 0..3
    }
    if (wave >= 4) {
#pragma unroll
        for (int j = 0; j < NT; ++j) red[wave - 4][j][lane] = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
        for (int j = 0; j < NT; ++j) { const float4 q = red[wave][j][lane]; red[wave][j][lane] = make_float4(acc[j][0] + q.x, acc[j][1] + q.y, acc[j][2] + q.z, acc[j][3] + q.w); }
    }
    __syncthreads();
    // final sum + bias, kept in red[0]: entry (j, lane) is read and written by one thread only
    for (int e = tid; e < NT * 64; e += ENV_WAVES * 64) {
        const int j = e >> 6, l = e & 63;
        float4 s = red[0][j][l];
#pragma unroll
        for (int w = 1; w < 4; ++w) { const float4 q = red[w][j][l]; s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w; }
        const float4 b = *reinterpret_cast<const float4*>(p.bias + j * 16 + (l >> 4) * 4);
        red[0][j][l] = make_float4(s.x + b.x, s.y + b.y, s.z + b.z, s.w + b.w);
    }
    __syncthreads();
    const float* hs = reinterpret_cast<const float*>(&red[0][0][0]);
    auto head = [&](int row, int c) { return hs[(((c >> 4) * 64) + ((c & 15) >> 2) * 16 + row) * 4 + (c & 3)]; };
    const int NO = p.NMIX * p.NDIM;
    const float q1 = 1e-5f, q2 = 1.f - 1e-5f;
    if (tid < 16 * p.NDIM) {               // one thread per (row, mixture dimension): Gumbel-max component choice + logistic inversion sample
        const int row = tid / p.NDIM, dd = tid - row * p.NDIM;
        const long long bs = r0 + row;
        if (bs < p.n) {
            int ksel = 0;
            float best = -INFINITY;
            for (int k = 0; k < p.NMIX; ++k) {
                const float u = p.u_mix ? p.u_mix[(bs * p.NDIM + dd) * p.NMIX + k] : hash_uniform(p.seed, (unsigned long long)((bs * p.NDIM + dd) * p.NMIX + k));
                const float g = head(row, dd * p.NMIX + k) - __logf(-__logf((q1 - q2) * u + q2));
                if (g > best) { best = g; ksel = k; }                     // first maximum, like torch.argmax
            }
            const float mu = head(row, NO + dd * p.NMIX + ksel);
            const float ls = fmaxf(head(row, 2 * NO + dd * p.NMIX + ksel), p.log_scale_min);
            const float uu = p.u_act ? p.u_act[bs * p.NDIM + dd] : hash_uniform(p.seed ^ 0x9e3779b97f4a7c15ull, (unsigned long long)(bs * p.NDIM + dd));
            const float u = (q1 - q2) * uu + q2;
            act_s[row][dd] = mu + __expf(ls) * (__logf(u) - __logf(1.f - u));
            if (dd == 0 && p.discrete_gripper) act_s[row][6] = (head(row, 3 * NO + 1) > head(row, 3 * NO)) ? 1.f : -1.f;      // gripper_bounds[argmax]
        }
    }
    __syncthreads();
    if (tid >= 16 || r0 + tid >= p.n) return;
    float a[7], w[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) a[i] = act_s[tid][i];
    if (p.gripper_control) {
        const float* ro = p.robot_obs + (long long)(r0 + tid) * 15;
        float R[9], Rr[9];
        env_euler_xyz(ro[3], ro[4], ro[5], R);
        env_euler_xyz(a[3] * 0.01f, a[4] * 0.01f, a[5] * 0.01f, Rr);
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
    } else {
#pragma unroll
        for (int i = 0; i < 7; ++i) w[i] = a[i];
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) p.pred[(long long)(r0 + tid) * 7 + i] = w[i];
}
// one workgroup per 16-row tile; NT = NHEAD / 16 accumulator tiles (192 packed head columns: hulc / gcbc, 224: mcil); byrow: the feed-forward body's row buffer
inline void launch_env_heads_sample(hipStream_t st, const EnvHeadsP& p, int NHEAD, bool byrow) {
    const dim3 grid((p.n + 15) / 16), block(ENV_WAVES * 64);
    if (NHEAD == 192 && byrow) hipLaunchKernelGGL((env_heads_sample_kernel<12, true>), grid, block, 0, st, p);
    else if (NHEAD == 192) hipLaunchKernelGGL((env_heads_sample_kernel<12>), grid, block, 0, st, p);
    else if (byrow) hipLaunchKernelGGL((env_heads_sample_kernel<14, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((env_heads_sample_kernel<14>), grid, block, 0, st, p);
}

// ---- slot state: store at plan time / install, gather for reads and for the fp32 engine's composed step ----------------------------------------------
struct EnvStoreP {
    const int* rowdesc; int n, max_envs;
    const int* pidx;                  // [n][NCAT] category indices (hulc) or null
    const float* plan_f;              // [n][PC] continuous plan (mcil) or null
    const void* goal;                 // [n][32] T
    int NCAT, NCLS, PC;
    int* s_plan_i; float* s_plan_f; void* s_goal;
    const void* wT;                   // W_ih0^T [KIN][2048] T, or null: no cache (fp32 engine)
    int grow0;                        // first goal row of wT
    const float *b1, *b2;
    float* s_cache;
    void *h0, *h1; int zero_hidden;
};
// grid (2048 / 256, n).  Block (bx, r): columns [256 bx, 256 bx + 256) of row r's slot — the cached decoder input term
//   cache[slot][i] = b_ih0[i] + b_hh0[i] + plan term + sum_k goal[r][k] W_ih0[i][goal col k]
// (plan term: the 32 gathered one-hot columns for hulc, sum_k plan[r][k] W_ih0[i][k] with the plan rounded to T for mcil, none for gcbc), both buffers of the two
// hidden states zeroed when the call clears them, and (bx == 0) the plan and goal values themselves.  A category index is clamped into [0, NCLS): it addresses memory.
template <typename T>
__global__ void __launch_bounds__(256) env_plan_store_kernel(EnvStoreP p) {
    __shared__ int sidx[64];
    __shared__ float sgoal[32];
    const int r = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const int slot = env_slot(p.rowdesc[r]);
    const T* goal = reinterpret_cast<const T*>(p.goal) + (long long)r * 32;
    if (p.pidx && tid < p.NCAT) sidx[tid] = min(max(p.pidx[r * p.NCAT + tid], 0), p.NCLS - 1);
    if (tid < 32) sgoal[tid] = to_f<T>(goal[tid]);
    __syncthreads();
    if (blockIdx.x == 0) {
        if (p.pidx && tid < p.NCAT) p.s_plan_i[slot * p.NCAT + tid] = sidx[tid];
        if (p.plan_f) for (int k = tid; k < p.PC; k += 256) p.s_plan_f[(long long)slot * p.PC + k] = p.plan_f[(long long)r * p.PC + k];
        if (tid < 32) reinterpret_cast<T*>(p.s_goal)[slot * 32 + tid] = goal[tid];
    }
    if (p.zero_hidden) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            reinterpret_cast<T*>(p.h0)[((long long)b * p.max_envs + slot) * ENV_HID + i] = from_f<T>(0.f);
            reinterpret_cast<T*>(p.h1)[((long long)b * p.max_envs + slot) * ENV_HID + i] = from_f<T>(0.f);
        }
    }
    if (!p.wT) return;
    const T* wT = reinterpret_cast<const T*>(p.wT);
    float s = p.b1[i] + p.b2[i];
    if (p.pidx) for (int c = 0; c < p.NCAT; ++c) s += to_f<T>(wT[(long long)(c * p.NCLS + sidx[c]) * ENV_HID + i]);
    if (p.plan_f) {
        float a = 0.f;
        for (int k = 0; k < p.PC; ++k) a += to_f<T>(from_f<T>(p.plan_f[(long long)r * p.PC + k])) * to_f<T>(wT[(long long)k * ENV_HID + i]);
        s += a;
    }
    float g = 0.f;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) g += sgoal[k] * to_f<T>(wT[(long long)(p.grow0 + k) * ENV_HID + i]);
    p.s_cache[(long long)slot * ENV_HID + i] = s + g;
}

struct EnvGatherP {
    const int* rowdesc; int n, max_envs, NCAT, PC;
    const int* s_plan_i; const float* s_plan_f; const void* s_goal; const void *h0, *h1;
    int* pidx; float* plan_f; void* plan_t; void* goal_t; float* goal_f; void *ha, *hb;      // every output optional
};
// grid (n): row r <- its slot's plan / goal (and, ha / hb given, the current hidden states h[parity][slot])
template <typename T>
__global__ void __launch_bounds__(256) env_gather_kernel(EnvGatherP p) {
    const int r = blockIdx.x, tid = threadIdx.x, d = p.rowdesc[r], slot = env_slot(d);
    if (p.pidx && tid < p.NCAT) p.pidx[r * p.NCAT + tid] = p.s_plan_i[slot * p.NCAT + tid];
    if (p.PC > 0) for (int k = tid; k < p.PC; k += 256) {
        const float v = p.s_plan_f[(long long)slot * p.PC + k];
        if (p.plan_f) p.plan_f[(long long)r * p.PC + k] = v;
        if (p.plan_t) reinterpret_cast<T*>(p.plan_t)[(long long)r * p.PC + k] = from_f<T>(v);
    }
    if (tid < 32) {
        const T g = reinterpret_cast<const T*>(p.s_goal)[slot * 32 + tid];
        if (p.goal_t) reinterpret_cast<T*>(p.goal_t)[r * 32 + tid] = g;
        if (p.goal_f) p.goal_f[r * 32 + tid] = to_f<T>(g);
    }
    if (p.ha) {
        const long long src = ((long long)env_par(d) * p.max_envs + slot) * ENV_HID;
        for (int k = tid; k < ENV_HID; k += 256) {
            reinterpret_cast<T*>(p.ha)[(long long)r * ENV_HID + k] = reinterpret_cast<const T*>(p.h0)[src + k];
            reinterpret_cast<T*>(p.hb)[(long long)r * ENV_HID + k] = reinterpret_cast<const T*>(p.h1)[src + k];
        }
    }
}
// grid (n): the composed step's new hidden states (rows of the call) -> h[1 - parity][slot]
template <typename T>
__global__ void __launch_bounds__(256) env_scatter_hidden_kernel(const int* __restrict__ rowdesc, int max_envs, const T* __restrict__ ha, const T* __restrict__ hb,
                                                                 T* __restrict__ h0, T* __restrict__ h1) {
    const int r = blockIdx.x, d = rowdesc[r];
    const long long dst = ((long long)(1 - env_par(d)) * max_envs + env_slot(d)) * ENV_HID;
    for (int k = threadIdx.x; k < ENV_HID; k += 256) { h0[dst + k] = ha[(long long)r * ENV_HID + k]; h1[dst + k] = hb[(long long)r * ENV_HID + k]; }
}
// grid (n): both buffers of both hidden states of the rows' slots <- 0
template <typename T>
__global__ void __launch_bounds__(256) env_zero_hidden_kernel(const int* __restrict__ rowdesc, int max_envs, T* __restrict__ h0, T* __restrict__ h1) {
    const int slot = env_slot(rowdesc[blockIdx.x]);
    for (int b = 0; b < 2; ++b)
        for (int k = threadIdx.x; k < ENV_HID; k += 256) { h0[((long long)b * max_envs + slot) * ENV_HID + k] = from_f<T>(0.f); h1[((long long)b * max_envs + slot) * ENV_HID + k] = from_f<T>(0.f); }
}

}  // namespace HULC_NS
