// hulc_amd/csrc/plan_ln_launch.h — the launch decisions of the kernels.h families as free functions of the stream (and, for the fp32 LayerNorm backward, the
// column-sum scratch): LayerNorm, the latent plan (sample + KL, its backward, gather, scatter), the action loss and sampler, the unfused attention, the 64-wide
// spatial softmax, the single-block sum.  Each helper owns its grid, block, dynamic LDS size and routing predicate (ln_bwd_fused, plan_scatter_w4, logistic_loss_wide,
// attention_wide / attention_s64) and is the ONLY place that launches its kernels: the engine (engine.h, engine_*.inc) and the per-kernel test entries (k_entries.h, capi.hip
// hulc_k_attention) call the same function, so an entry runs a kernel exactly as the engine does.
#pragma once
#include <algorithm>
#include <type_traits>
#include "kernels.h"

namespace HULC_NS {

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

template <typename T>
inline void launch_ln_fwd(hipStream_t st, const float* x, long long ldx, int rows, int n, const float* g, const float* b, T* out, long long ldo, float* outf,
                          long long ldf, float* stats) {
    hipLaunchKernelGGL((layernorm_fwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, st, x, ldx, rows, n, g, b, out, ldo, outf, ldf, stats);
}
// the fused backward serves the 16-bit types only; its broadcast / partial-sum forms of dy exist nowhere else
template <typename T> constexpr bool ln_bwd_fused() { return std::is_same<T, h16_t>::value; }
inline int ln_bwd_rows_per_block(int rows) { return rows >= 1024 ? 16 : 4; }          // fused: 16 rows and 16 waves per block from 1024 rows on
inline int ln_bwd_nsplit(int rows) { return std::max(1, std::min(64, cdiv(rows, 64))); }          // fp32 pair: row chunks of the parameter gradients
inline long long ln_bwd_scratch_floats(int rows, int n) { return 2ll * ln_bwd_nsplit(rows) * n; }          // [2][nsplit][n] partial sums (fp32 pair only)
// bcast_rows > 0 (fused kernel only): dy holds one row per WINDOW, broadcast over its bcast_rows rows and divided by bcast_div
template <typename T>
inline void launch_ln_bwd(hipStream_t st, float* scratch, const float* dy, long long lddy, const float* x, long long ldx, const float* stats, const float* g, int rows,
                          int n, float* dxf, long long ldd, int acc, T* dxt, long long ldt, float* dg, float* db, float drop_p = 0.f, unsigned long long drop_seed = 0,
                          int bcast_rows = 0, float bcast_div = 1.f, int dy_parts = 1, long long dy_part_stride = 0, bool fixed_order = false) {
    if constexpr (ln_bwd_fused<T>()) {
        const int rpb = ln_bwd_rows_per_block(rows);
        const int nblk = cdiv(rows, rpb);
        // fixed_order (reproducible mode): the blocks store their gamma / beta partials in `scratch` ([2][nblk][n]) and the fp32 pair's second stage adds them in block order
        const bool slab = fixed_order && dg && nblk > 1;
        hipLaunchKernelGGL((layernorm_bwd_fused_kernel<T>), dim3(nblk), dim3(rpb == 16 ? 1024 : 256), 0, st, dy, lddy, x, ldx, stats, g, rows, n, dxf, ldd, acc, dxt, ldt,
                           drop_p, drop_seed, rpb, dg, db, bcast_rows, bcast_div, dy_parts, dy_part_stride, slab ? scratch : (float*)nullptr);
        if (slab) {
            hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch, nblk, n, dg, (float*)nullptr, 1.f);
            hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch + (long long)nblk * n, nblk, n, db, (float*)nullptr, 1.f);
        }
    } else {        // fp32 (parity) mode: unfused and deterministic
        if ((drop_p > 0.f || drop_seed != 0) && dxt && dxf) {       // dx first, its copy through the dropout mask in a second launch
            hipLaunchKernelGGL((layernorm_bwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, st, dy, lddy, x, ldx, stats, g, rows, n, dxf, ldd, acc, (T*)nullptr, 0);
            hipLaunchKernelGGL((dropout_apply_kernel<T>), dim3(cdiv((long long)rows * n, 256)), dim3(256), 0, st, dxf, (float*)nullptr, dxt, (long long)rows * n, drop_p, drop_seed);
        } else
            hipLaunchKernelGGL((layernorm_bwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, st, dy, lddy, x, ldx, stats, g, rows, n, dxf, ldd, acc, dxt, ldt);
        const int nsplit = ln_bwd_nsplit(rows);
        hipLaunchKernelGGL(layernorm_param_grad_kernel, dim3(cdiv(n, 64), nsplit), dim3(256), 0, st, dy, lddy, x, ldx, stats, rows, n, cdiv(rows, nsplit), scratch, (float*)nullptr, (float*)nullptr);
        hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch, nsplit, n, dg, (float*)nullptr, 1.f);
        hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch + (long long)nsplit * n, nsplit, n, db, (float*)nullptr, 1.f);
    }
}

// 16-bit engines: four waves per tile (and stores into a fresh buffer); the fp32 engine keeps the serial sum order.  Both kernels hold NCLS <= 32 rows in LDS.
template <typename T> inline bool plan_scatter_w4(int NCLS) { return !std::is_same<T, float>::value && NCLS <= 32; }
template <typename T>
inline void launch_plan_scatter_grad(hipStream_t st, bool w4, const T* dC, const int* idx, int B, int NCAT, int NCLS, int H, int KIN, float* dw, int store) {
    if (w4) hipLaunchKernelGGL((plan_scatter_grad_w4_kernel<T>), dim3(NCAT, cdiv(H, 64)), dim3(256), 0, st, dC, idx, B, NCAT, NCLS, H, KIN, dw, store);
    else hipLaunchKernelGGL((plan_scatter_grad_lds_kernel<T>), dim3(NCAT, cdiv(H, 64)), dim3(64), 0, st, dC, idx, B, NCAT, NCLS, H, KIN, dw);
}

// ---- latent plan: sample + KL (one wave per (b, category)), the backward of the sample, the one-hot gather ------------------------------------------------------
inline void launch_plan_kl_sample(hipStream_t st, const float* pr_logits, const float* pp_logits, int B, int NCAT, int NCLS, const int* idx_in, int* idx_out, float* probs,
                                  float* kl_cat, float* dpp, float* dpr, float w_pp, float w_pr, unsigned long long seed, const float* lscale) {
    hipLaunchKernelGGL(plan_kl_sample_kernel, dim3(B * NCAT), dim3(64), 0, st, pr_logits, pp_logits, B, NCAT, NCLS, idx_in, idx_out, probs, kl_cat, dpp, dpr, w_pp, w_pr, seed, lscale);
}
template <typename T>
inline void launch_st_softmax_bwd(hipStream_t st, const float* probs, const float* dplan, const float* dpr_kl, const float* dpp_kl, int rows, int NCLS, float* out, T* out_t, T* dpp_t) {
    hipLaunchKernelGGL((st_softmax_bwd_kernel<T>), dim3(rows), dim3(64), 0, st, probs, dplan, dpr_kl, NCLS, out, out_t, dpp_kl, dpp_t);
}
template <typename T>
inline void launch_normal_kl_sample(hipStream_t st, const float* pr_state, const float* pp_state, int B, int n, const float* eps_in, float* eps_out, float* plan_f, T* plan_t,
                                    float* kl_elem, float* dpp, float* dpr, float w_pp, float w_pr, unsigned long long seed, const float* lscale) {
    hipLaunchKernelGGL((normal_kl_sample_kernel<T>), dim3(cdiv((long long)B * n, 256)), dim3(256), 0, st, pr_state, pp_state, B, n, eps_in, eps_out, plan_f, plan_t, kl_elem, dpp,
                       dpr, w_pp, w_pr, seed, lscale);
}
template <typename T>
inline void launch_normal_rsample_bwd(hipStream_t st, const float* dplan, const float* eps, const float* pr_state, const float* dpr_kl, int B, int n, T* out) {
    hipLaunchKernelGGL((normal_rsample_bwd_kernel<T>), dim3(cdiv((long long)B * n, 256)), dim3(256), 0, st, dplan, eps, pr_state, dpr_kl, B, n, out);
}
// a two-part grid: the blocks of the gather (and of cb, the goal term), then those of the time-major copy emb -> embg (none without embg: S = W = 0)
template <typename T>
inline void launch_plan_gather(hipStream_t st, const T* w_t, const int* idx, int B, int NCAT, int NCLS, int H, const float* b1, const float* b2, float* out, const T* emb, T* embg,
                               int S, int W, const T* goal, int G, int grow0, T* cb) {
    hipLaunchKernelGGL((plan_gather_t_kernel<T>), dim3(cdiv((long long)B * H, 256) + cdiv((long long)S * B * W, 256)), dim3(256), 0, st, w_t, idx, B, NCAT, NCLS, H, b1, b2, out, emb,
                       embg, S, W, goal, G, grow0, cb);
}
// LayerNorm of [B][S][n] and its mean over S: one 1024-thread block per window
template <typename T>
inline void launch_ln_mean(hipStream_t st, const float* x, int B, int S, int n, const float* g, const float* b, float* stats, T* out, float* yout) {
    hipLaunchKernelGGL((layernorm_mean_kernel<T>), dim3(B), dim3(1024), 0, st, x, S, n, g, b, stats, out, yout);
}
// ---- action loss and sampler ---------------------------------------------------------------------------------------------------------------------------------
static constexpr int LL_NMIX = 10;      // the serial loss kernel's compile-time mixture count (Engine::NMIX)
// 16-bit engines: one lane per mixture component (logistic_loss_wide_kernel: 17.9 -> ~6 us); the fp32 parity engine keeps the serial kernel's summation order
template <typename T> inline bool logistic_loss_wide(int nmix, int ndim) { return !std::is_same<T, float>::value && nmix <= 16 && ndim <= 7; }
// serial (nmix == LL_NMIX): one thread per (row, slot of 8), one long chain each; one wave per workgroup: 256 CUs x 1 wave instead of 64 CUs x 4
template <typename T>
inline void launch_logistic_loss(hipStream_t st, bool wide, const float* heads, int ldh, const float* actions, const float* robot_obs, int B, int S, int nmix, int ndim,
                                 int num_classes, float log_scale_min, float gripper_alpha, int gripper_control, int discrete_gripper, float grad_scale, const float* lscale,
                                 float* row_loss, float* a_tcp_out, T* dheads) {
    if (wide) hipLaunchKernelGGL((logistic_loss_wide_kernel<T>), dim3(S * B), dim3(128), 0, st, heads, ldh, actions, robot_obs, B, S, nmix, ndim, num_classes, log_scale_min,
                                 gripper_alpha, gripper_control, grad_scale, row_loss, a_tcp_out, dheads, discrete_gripper, lscale);
    else hipLaunchKernelGGL((logistic_loss_kernel<T, LL_NMIX>), dim3(cdiv((long long)S * B * 8, 64)), dim3(64), 0, st, heads, ldh, actions, robot_obs, B, S, nmix, ndim, num_classes,
                            log_scale_min, gripper_alpha, gripper_control, grad_scale, row_loss, a_tcp_out, dheads, discrete_gripper, lscale);
}
// one thread per row (b, t), one wave per workgroup
inline void launch_logistic_sample(hipStream_t st, const float* heads, int ldh, const float* robot_obs, const float* actions_gt, const float* u_mix, const float* u_act, int B, int S,
                                   int nmix, int ndim, float log_scale_min, int gripper_control, int discrete_gripper, unsigned long long seed, float* pred_out, float* metrics) {
    hipLaunchKernelGGL(logistic_sample_kernel, dim3(cdiv((long long)B * S, 64)), dim3(64), 0, st, heads, ldh, robot_obs, actions_gt, u_mix, u_act, B, S, nmix, ndim, log_scale_min,
                       gripper_control, seed, pred_out, metrics, discrete_gripper);
}
// out[0] = scale * sum(x[0 .. n)): a single block, a fixed tree
inline void launch_sum_reduce(hipStream_t st, const float* x, int n, float scale, float* out) {
    hipLaunchKernelGGL(sum_reduce_kernel, dim3(1), dim3(256), 0, st, x, n, scale, out);
}
// ---- unfused attention, one workgroup per (b, head) ------------------------------------------------------------------------------------------------------------
// The form is (WIDE, s64).  WIDE: two lanes per query row (attention_*32_kernel, S <= 32) or, with s64, four waves (attention_*64_kernel, any S <= 64); !WIDE: one lane per
// query row, attention_*_kernel<T, 32 / 64>, float only.  The engines' rule: attention_wide<T>(), attention_s64(S) — the fp32 (parity) engine keeps the one-lane kernel's summation
// order: the hulc_visonly fixture has an FFN pre-activation within fp32 epsilon of zero, and an epsilon-level change upstream flips its ReLU (1e-3 gradient gate)
template <typename T> constexpr bool attention_wide() { return !std::is_same<T, float>::value; }
inline bool attention_s64(int S) { return S > 32; }
template <typename T, bool WIDE = attention_wide<T>()>
inline void launch_attention_fwd(hipStream_t st, bool s64, const T* qkv, int B, int S, int D, int NH, float* P, T* ao, float drop_p, unsigned long long seed) {
    static_assert(WIDE || std::is_same<T, float>::value, "the one-lane attention kernels are instantiated for float only");
    const dim3 grid(B * NH);
    if constexpr (WIDE) {
        if (!s64) hipLaunchKernelGGL((attention_fwd32_kernel<T>), grid, dim3(64), 0, st, qkv, B, S, D, NH, P, ao, drop_p, seed);
        else hipLaunchKernelGGL((attention_fwd64_kernel<T>), grid, dim3(256), 0, st, qkv, B, S, D, NH, P, ao, drop_p, seed);
    } else if (!s64) hipLaunchKernelGGL((attention_fwd_kernel<T, 32>), grid, dim3(64), 0, st, qkv, B, S, D, NH, P, ao, drop_p, seed);
    else hipLaunchKernelGGL((attention_fwd_kernel<T, 64>), grid, dim3(64), 0, st, qkv, B, S, D, NH, P, ao, drop_p, seed);
}
template <typename T, bool WIDE = attention_wide<T>()>
inline void launch_attention_bwd(hipStream_t st, bool s64, const T* qkv, const float* P, const T* dao, int B, int S, int D, int NH, T* dqkv, float drop_p, unsigned long long seed) {
    static_assert(WIDE || std::is_same<T, float>::value, "the one-lane attention kernels are instantiated for float only");
    const dim3 grid(B * NH);
    if constexpr (WIDE) {
        if (!s64) hipLaunchKernelGGL((attention_bwd32_kernel<T>), grid, dim3(64), 0, st, qkv, P, dao, B, S, D, NH, dqkv, drop_p, seed);
        else {      // ATT_BWD64_LDS (99.5 KB, dynamic) is past the default limit: raised once per instantiation
            max_dyn_lds_once<&attention_bwd64_kernel<T>>((int)ATT_BWD64_LDS);
            hipLaunchKernelGGL((attention_bwd64_kernel<T>), grid, dim3(256), ATT_BWD64_LDS, st, qkv, P, dao, B, S, D, NH, dqkv, drop_p, seed);
        }
    } else if (!s64) hipLaunchKernelGGL((attention_bwd_kernel<T, 32>), grid, dim3(64), 0, st, qkv, P, dao, B, S, D, NH, dqkv, drop_p, seed);
    else hipLaunchKernelGGL((attention_bwd_kernel<T, 64>), grid, dim3(64), 0, st, qkv, P, dao, B, S, D, NH, dqkv, drop_p, seed);
}
// ---- the 64-channel spatial softmax of the 16-bit encoder head: one block per frame ------------------------------------------------------------------------------
inline void launch_spatial_softmax64_fwd(hipStream_t st, const h16_t* f, int Nf, int H, int W, h16_t* out, float* stats) {
    hipLaunchKernelGGL(spatial_softmax_fwd64_kernel, dim3(Nf), dim3(256), 0, st, f, H, W, out, stats);
}
inline void launch_spatial_softmax64_bwd(hipStream_t st, const h16_t* f, const float* stats, const float* dout, int Nf, int H, int W, h16_t* df) {
    hipLaunchKernelGGL(spatial_softmax_bwd64_kernel, dim3(Nf), dim3(256), 0, st, f, stats, dout, H, W, df);
}

}  // namespace HULC_NS
