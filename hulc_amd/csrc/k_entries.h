// hulc_amd/csrc/k_entries.h — per-kernel test entries of the 16-bit encoder head and of the action loss (include/hulc_hip.h: hulc_k_spatial_softmax64,
// hulc_k_enc_tail_fwd, hulc_k_enc_tail_bwd, hulc_k_logistic_loss), of the latent-plan kernels (hulc_k_plan_*, hulc_k_st_softmax_bwd, hulc_k_normal_*), of
// the LayerNorm family (hulc_k_layernorm_*) and of the fused transformer layer kernels
// (hulc_k_tr_layer_fwd, hulc_k_tr_ffn_bwd, hulc_k_tr_attn_bwd; launched through tr_fused.h's helpers), and of the GEMM core with its runtime epilogue
// (hulc_k_gemm_epi, hulc_k_gemm_dual, hulc_k_gemm_pick, hulc_k_gemm_wgrad_nsplit; launched through gemm.h's launchers and routing), and of the encoder's convolution family
// (hulc_k_conv_tile, hulc_k_conv_pair, hulc_k_conv_wgrad, hulc_k_conv1_wgrad_u8 and their per-type forms; launched through the launchers of conv_tile.h, conv_reg.h,
// conv_wgrad.h and conv1_wgrad.h).  Included by engine.h inside each translation unit, so every entry exists once per
// 16-bit type (hulc_bf16 / hulc_f16; iengine.h declares them).  Nothing here restates a kernel or a launch: every entry checks its arguments, then launches
// through the helper the engine calls (plan_ln_launch.h for the kernels.h families, enc_tail.h, det_head.h, tr_fused.h, gemm.h, the conv launchers).
#pragma once
#include "iengine.h"
#include "kernels.h"
#include "enc_tail.h"
#include "plan_ln_launch.h"
#include "gemm.h"
#include "tr_fused.h"
#include "det_head.h"
#include <vector>

namespace HULC_NS {

static inline bool k_misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static inline int k_launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { hulc_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return 1; }
    return 0;
}

// dout == null: the forward (f -> out, stats); dout given: the backward (f, stats, dout -> df)
int k_spatial_softmax64(const void* f, int H, int W, int Nf, void* out, float* stats, const float* dout, void* df, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (Nf < 1 || H < 2 || W < 2 || (long long)H * W > (1 << 20)) { hulc_set_error("hulc_k_spatial_softmax64: Nf=%d H=%d W=%d (need Nf >= 1, H, W >= 2)", Nf, H, W); return 1; }
    if (!f || !stats || (dout ? !df : !out)) { hulc_set_error("hulc_k_spatial_softmax64: null argument"); return 1; }
    if (k_misaligned16(f) || k_misaligned16(stats) || k_misaligned16(dout) || k_misaligned16(df)) { hulc_set_error("hulc_k_spatial_softmax64: f, stats, dout, df must be 16-byte aligned"); return 1; }
    if (!dout) launch_spatial_softmax64_fwd(st, (const h16_t*)f, Nf, H, W, (h16_t*)out, stats);
    else launch_spatial_softmax64_bwd(st, (const h16_t*)f, stats, dout, Nf, H, W, (h16_t*)df);
    return k_launched("hulc_k_spatial_softmax64");
}

int k_enc_tail_fwd(int Nf, int ldemb, const hulc_enc_tail_job* a, const hulc_enc_tail_job* b, void* emb, const float* pos, int S, float drop_p,
                   unsigned long long seed, float* xf, void* xt, float* z0, float* z1, void* stream) {
    if (Nf < 1 || ldemb < 64 || !a || !b || !emb) { hulc_set_error("hulc_k_enc_tail_fwd: Nf=%d ldemb=%d or a null argument", Nf, ldemb); return 1; }
    if (pos && (S < 1 || !(drop_p >= 0.f && drop_p < 1.f) || !xf || !xt || !z0 || !z1)) {
        hulc_set_error("hulc_k_enc_tail_fwd: pos given: need S >= 1 (S=%d), 0 <= drop_p < 1 and xf, xt, z0, z1", S); return 1;
    }
    EncTailP q{};
    const hulc_enc_tail_job* jobs[2] = {a, b};
    for (int k = 0; k < 2; ++k) {
        const hulc_enc_tail_job& j = *jobs[k];
        if (!j.x || !j.W1 || !j.W2 || !j.b1 || !j.b2 || !j.lng || !j.lnb || !j.f1 || !j.f2 || !j.lnst) { hulc_set_error("hulc_k_enc_tail_fwd: job %d has a null pointer", k); return 1; }
        if (j.col0 < 0 || j.col0 + 64 > ldemb) { hulc_set_error("hulc_k_enc_tail_fwd: job %d col0=%d outside ldemb=%d", k, (int)j.col0, ldemb); return 1; }
        if (k_misaligned16(j.x) || k_misaligned16(j.W1) || k_misaligned16(j.W2) || k_misaligned16(j.b1) || k_misaligned16(j.b2) || k_misaligned16(j.f1)) {
            hulc_set_error("hulc_k_enc_tail_fwd: job %d: x, W1, W2, b1, b2, f1 must be 16-byte aligned", k); return 1;
        }
        EncTailCam& c = q.cam[k];
        c.x = (const h16_t*)j.x; c.W1 = (const h16_t*)j.W1; c.W2 = (const h16_t*)j.W2; c.b1 = j.b1; c.b2 = j.b2; c.lng = j.lng; c.lnb = j.lnb;
        c.f1 = (h16_t*)j.f1; c.f2 = j.f2; c.lnst = j.lnst; c.col0 = j.col0;
    }
    q.emb = (h16_t*)emb; q.Nf = Nf; q.ldemb = ldemb;
    if (pos) { q.pos = pos; q.xf = xf; q.xt = (h16_t*)xt; q.z0 = z0; q.z1 = z1; q.S = S; q.drop_p = drop_p; q.seed = seed; }
    launch_enc_tail_fwd((hipStream_t)stream, q);
    return k_launched("hulc_k_enc_tail_fwd");
}

int k_enc_tail_bwd(int Nf, int ldemb, const hulc_enc_tail_bwd_job* a, const hulc_enc_tail_bwd_job* b, const float* demb, void* stream) {
    if (Nf < 1 || ldemb < 64 || !a || !b || !demb) { hulc_set_error("hulc_k_enc_tail_bwd: Nf=%d ldemb=%d or a null argument", Nf, ldemb); return 1; }
    EncTailBwdP q{};
    const hulc_enc_tail_bwd_job* jobs[2] = {a, b};
    for (int k = 0; k < 2; ++k) {
        const hulc_enc_tail_bwd_job& j = *jobs[k];
        if (!j.f2 || !j.lnst || !j.lng || !j.f1 || !j.W2t || !j.W1t || !j.dlng || !j.dlnb || !j.d_f2 || !j.d_f1) { hulc_set_error("hulc_k_enc_tail_bwd: job %d has a null pointer", k); return 1; }
        if (!j.dx_f32 == !j.dx_t) { hulc_set_error("hulc_k_enc_tail_bwd: job %d needs exactly one of dx_f32 (fp32, unmasked) and dx_t (16 bit)", k); return 1; }
        if (j.dx_f32 && j.xmask) { hulc_set_error("hulc_k_enc_tail_bwd: job %d: xmask goes with dx_t", k); return 1; }
        if (j.col0 < 0 || j.col0 + 64 > ldemb) { hulc_set_error("hulc_k_enc_tail_bwd: job %d col0=%d outside ldemb=%d", k, (int)j.col0, ldemb); return 1; }
        if (k_misaligned16(j.W2t) || k_misaligned16(j.W1t) || k_misaligned16(j.f1) || k_misaligned16(j.d_f1) || k_misaligned16(j.xmask) || k_misaligned16(j.dx_f32) || k_misaligned16(j.dx_t)) {
            hulc_set_error("hulc_k_enc_tail_bwd: job %d: W2t, W1t, f1, d_f1, xmask, dx must be 16-byte aligned", k); return 1;
        }
        EncTailBwdCam& c = q.cam[k];
        c.f2 = j.f2; c.lnst = j.lnst; c.lng = j.lng; c.f1 = (const h16_t*)j.f1; c.W2t = (const h16_t*)j.W2t; c.W1t = (const h16_t*)j.W1t; c.xmask = (const h16_t*)j.xmask;
        c.dlng = j.dlng; c.dlnb = j.dlnb; c.d_f2 = (h16_t*)j.d_f2; c.d_f1 = (h16_t*)j.d_f1; c.dx_f32 = j.dx_f32; c.dx_t = (h16_t*)j.dx_t; c.col0 = j.col0;
    }
    q.demb = demb; q.Nf = Nf; q.ldemb = ldemb;
    launch_enc_tail_bwd((hipStream_t)stream, q);
    return k_launched("hulc_k_enc_tail_bwd");
}

// t16 of the typed entries: 0 = float, 1 = this translation unit's 16-bit type (the fp32 instances live in the bf16 unit).  HULC_K_T runs the launch, an
// expression over the element type TT, for the selected type
#ifdef HULC_HALF_F16
#define HULC_K_T(who, ...) do { if (t16) { using TT = h16_t; __VA_ARGS__; } else { hulc_set_error(who ": the fp32 instances live in the bf16 translation unit"); return 1; } } while (0)
#else
#define HULC_K_T(who, ...) do { if (t16) { using TT = h16_t; __VA_ARGS__; } else { using TT = float; __VA_ARGS__; } } while (0)
#endif
int k_logistic_loss(int t16, int wide, const float* heads, int ldh, const float* actions, const float* robot_obs, int B, int S, int nmix, int ndim, int num_classes,
                    float log_scale_min, float gripper_alpha, int gripper_control, int discrete_gripper, float grad_scale, const float* lscale, float* row_loss, float* a_tcp_out,
                    void* dheads, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || S < 1 || (long long)B * S > (1 << 24) || nmix != LL_NMIX || ndim < 1 || ndim > (discrete_gripper ? 6 : 7) || num_classes < 2) {
        hulc_set_error("hulc_k_logistic_loss: B=%d S=%d nmix=%d (must be %d) ndim=%d (1..%d) num_classes=%d", B, S, nmix, LL_NMIX, ndim, discrete_gripper ? 6 : 7, num_classes); return 1;
    }
    if (ldh < 3 * nmix * ndim + (discrete_gripper ? 2 : 0)) { hulc_set_error("hulc_k_logistic_loss: ldh=%d narrower than the heads", ldh); return 1; }
    if (!heads || !actions || !row_loss || !dheads || (gripper_control && !robot_obs)) { hulc_set_error("hulc_k_logistic_loss: null argument"); return 1; }
    HULC_K_T("hulc_k_logistic_loss", launch_logistic_loss<TT>(st, wide != 0, heads, ldh, actions, robot_obs, B, S, nmix, ndim, num_classes, log_scale_min, gripper_alpha, gripper_control,
                                                               discrete_gripper, grad_scale, lscale, row_loss, a_tcp_out, (TT*)dheads));
    return k_launched("hulc_k_logistic_loss");
}

// ---------------------------------------------------------------------------------------------------- latent plan + LayerNorm
static inline bool k_misaligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) != 0; }
// plan indices address LDS rows and weight rows unchecked inside the kernels: the entry reads them back (a synchronous copy) and refuses any outside [0, NCLS)
static int k_idx_out_of_range(const char* who, const int* idx, long long count, int NCLS, hipStream_t st) {
    std::vector<int> h((size_t)count);
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h.data(), idx, sizeof(int) * (size_t)count, hipMemcpyDefault) != hipSuccess) {
        hulc_set_error("%s: the plan indices could not be read", who); return 1;
    }
    for (long long i = 0; i < count; ++i)
        if (h[i] < 0 || h[i] >= NCLS) { hulc_set_error("%s: plan index %d at position %lld is outside [0, %d)", who, h[i], i, NCLS); return 1; }
    return 0;
}

// ---------------------------------------------------------------------------------------------------- deterministic decoder head (det_head.h)
static inline bool k_det_shape_bad(const char* who, int B, int S) {
    if (B < 1 || S < 1 || (long long)B * S > (1 << 22)) { hulc_set_error("%s: B=%d S=%d (need B, S >= 1 and B*S <= 2^22)", who, B, S); return true; }
    return false;
}
int k_det_head_loss(int t16, const void* H1, const void* W, const float* bias, const float* actions, const float* robot_obs, int B, int S, int criterion, int frame,
                    float grad_scale, const float* lscale, float* row_loss, float* pred, float* dpre, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (k_det_shape_bad("hulc_k_det_head_loss", B, S)) return 1;
    if ((criterion != HULC_CRIT_HUBER && criterion != HULC_CRIT_MSE) || (frame != 0 && frame != 1)) { hulc_set_error("hulc_k_det_head_loss: criterion=%d frame=%d (both 0 or 1)", criterion, frame); return 1; }
    if (!H1 || !W || !bias || !actions || !robot_obs || !row_loss || !pred || !dpre) { hulc_set_error("hulc_k_det_head_loss: null argument"); return 1; }
    if (k_misaligned(H1, 16) || k_misaligned(W, 16) || k_misaligned(dpre, 16) || k_misaligned(bias, 4) || k_misaligned(actions, 4) || k_misaligned(robot_obs, 4) ||
        k_misaligned(lscale, 4) || k_misaligned(row_loss, 4) || k_misaligned(pred, 4)) { hulc_set_error("hulc_k_det_head_loss: misaligned pointer (H1, W, dpre: 16 bytes; the rest: 4)"); return 1; }
    HULC_K_T("hulc_k_det_head_loss", launch_det_head_loss<TT>(st, (const TT*)H1, (const TT*)W, bias, actions, robot_obs, B, S, criterion, frame, grad_scale, lscale, row_loss, 1, pred, dpre));
    return k_launched("hulc_k_det_head_loss");
}
int k_det_head_bwd(int t16, const float* dpre, const void* W, const void* H1, int B, int S, void* dH1, void* dZ1, float* dW, float* db, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (k_det_shape_bad("hulc_k_det_head_bwd", B, S)) return 1;
    if (!dpre || !W || !H1 || !dH1 || !dZ1 || !dW || !db) { hulc_set_error("hulc_k_det_head_bwd: null argument"); return 1; }
    if (k_misaligned(dpre, 16) || k_misaligned(W, 16) || k_misaligned(H1, 16) || k_misaligned(dH1, 16) || k_misaligned(dZ1, 16) || k_misaligned(dW, 4) || k_misaligned(db, 4)) {
        hulc_set_error("hulc_k_det_head_bwd: misaligned pointer (dpre, W, H1, dH1, dZ1: 16 bytes; dW, db: 4)"); return 1; }
    float* part = nullptr;
    if (hipMalloc((void**)&part, sizeof(float) * (size_t)det_head_slabs(B * S) * DET_SLAB) != hipSuccess) { hulc_set_error("hulc_k_det_head_bwd: hipMalloc failed"); return 1; }
#define HULC_K_L(TT)                                                                                                     \
    do {                                                                                                                 \
        launch_det_head_dgrad<TT>(st, dpre, (const TT*)W, (const TT*)H1, B, S, (TT*)dH1, (TT*)dZ1);                       \
        launch_det_head_wgrad<TT>(st, dpre, (const TT*)H1, B * S, part, dW, db);                                         \
    } while (0)
#ifdef HULC_HALF_F16
    if (!t16) { hipFree(part); hulc_set_error("hulc_k_det_head_bwd: the fp32 instances live in the bf16 translation unit"); return 1; }
    HULC_K_L(h16_t);
#else
    if (t16) HULC_K_L(h16_t); else HULC_K_L(float);
#endif
#undef HULC_K_L
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    hipFree(part);
    if (e1 != hipSuccess || e2 != hipSuccess) { hulc_set_error("hulc_k_det_head_bwd: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2)); return 1; }
    return 0;
}
int k_det_head_act(int t16, const void* h1, const void* W, const float* bias, const float* robot_obs, int n, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (k_det_shape_bad("hulc_k_det_head_act", n, 1)) return 1;
    if (!h1 || !W || !bias || !robot_obs || !out) { hulc_set_error("hulc_k_det_head_act: null argument"); return 1; }
    if (k_misaligned(h1, 16) || k_misaligned(W, 16) || k_misaligned(bias, 4) || k_misaligned(robot_obs, 4) || k_misaligned(out, 4)) {
        hulc_set_error("hulc_k_det_head_act: misaligned pointer (h1, W: 16 bytes; the rest: 4)"); return 1; }
    HULC_K_T("hulc_k_det_head_act", launch_det_head_act<TT>(st, (const TT*)h1, nullptr, 0, (const TT*)W, bias, robot_obs, nullptr, n, 1, out, nullptr));
    return k_launched("hulc_k_det_head_act");
}

int k_plan_kl_sample(const float* pr_logits, const float* pp_logits, int B, int NCAT, int NCLS, const int* idx_in, int* idx_out, float* probs, float* kl_cat, float* dpp,
                     float* dpr, float w_pp, float w_pr, unsigned long long seed, const float* lscale, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || NCAT < 1 || NCLS < 1 || NCLS > 64 || (long long)B * NCAT * NCLS > (1ll << 30)) { hulc_set_error("hulc_k_plan_kl_sample: B=%d NCAT=%d NCLS=%d (need B, NCAT >= 1 and 1 <= NCLS <= 64)", B, NCAT, NCLS); return 1; }
    if (!pr_logits || !idx_out || !probs || (pp_logits && (!kl_cat || !dpp || !dpr))) { hulc_set_error("hulc_k_plan_kl_sample: null argument"); return 1; }
    if (k_misaligned(pr_logits, 4) || k_misaligned(pp_logits, 4) || k_misaligned(idx_in, 4) || k_misaligned(idx_out, 4) || k_misaligned(probs, 4) || k_misaligned(kl_cat, 4) ||
        k_misaligned(dpp, 4) || k_misaligned(dpr, 4) || k_misaligned(lscale, 4)) { hulc_set_error("hulc_k_plan_kl_sample: every pointer must be 4-byte aligned"); return 1; }
    if (idx_in && k_idx_out_of_range("hulc_k_plan_kl_sample", idx_in, (long long)B * NCAT, NCLS, st)) return 1;
    launch_plan_kl_sample(st, pr_logits, pp_logits, B, NCAT, NCLS, idx_in, idx_out, probs, kl_cat, dpp, dpr, w_pp, w_pr, seed, lscale);
    return k_launched("hulc_k_plan_kl_sample");
}

int k_st_softmax_bwd(int t16, const float* probs, const float* dplan, const float* dpr_kl, const float* dpp_kl, int rows, int NCLS, float* out, void* out_t, void* dpp_t,
                     void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (rows < 1 || NCLS < 1 || NCLS > 64 || (long long)rows * NCLS > (1ll << 30)) { hulc_set_error("hulc_k_st_softmax_bwd: rows=%d NCLS=%d (need rows >= 1 and 1 <= NCLS <= 64)", rows, NCLS); return 1; }
    if (!probs || !dplan || !dpr_kl || !dpp_kl || !out || !out_t || !dpp_t) { hulc_set_error("hulc_k_st_softmax_bwd: null argument"); return 1; }
    const int ta = t16 ? 2 : 4;
    if (k_misaligned(probs, 4) || k_misaligned(dplan, 4) || k_misaligned(dpr_kl, 4) || k_misaligned(dpp_kl, 4) || k_misaligned(out, 4) || k_misaligned(out_t, ta) || k_misaligned(dpp_t, ta)) {
        hulc_set_error("hulc_k_st_softmax_bwd: a pointer is not aligned to its element type"); return 1;
    }
    HULC_K_T("hulc_k_st_softmax_bwd", launch_st_softmax_bwd<TT>(st, probs, dplan, dpr_kl, dpp_kl, rows, NCLS, out, (TT*)out_t, (TT*)dpp_t));
    return k_launched("hulc_k_st_softmax_bwd");
}

// embg == null: S = W = 0, no trailing blocks (the engine's grid always carries them; without the copy they have nothing to do).  The rows grow0 .. grow0 + G - 1 of
// w_t and its plan rows 0 .. NCAT * NCLS - 1 are the caller's to provide.
int k_plan_gather(int t16, const void* w_t, const int* idx, int B, int NCAT, int NCLS, int H, const float* b1, const float* b2, float* out, const void* emb, void* embg, int S,
                  int W, const void* goal, int G, int grow0, void* cb, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || H < 256 || (H % 256) != 0 || NCAT < 0 || NCAT > 64 || NCLS < 1 || (long long)B * H > (1ll << 30)) {
        hulc_set_error("hulc_k_plan_gather: B=%d H=%d NCAT=%d NCLS=%d (need B >= 1, H a multiple of 256, 0 <= NCAT <= 64, NCLS >= 1)", B, H, NCAT, NCLS); return 1;
    }
    if (!w_t || !b1 || !b2 || !out || (NCAT > 0 && !idx) || (!emb != !embg) || (cb && !goal)) { hulc_set_error("hulc_k_plan_gather: null argument (emb and embg go together, cb needs goal)"); return 1; }
    if (embg && (S < 1 || W < 1 || W > 128 || (long long)S * B * W > (1ll << 30))) { hulc_set_error("hulc_k_plan_gather: embg given: S=%d W=%d (need S >= 1, 1 <= W <= 128)", S, W); return 1; }
    if (cb && (G < 1 || grow0 < NCAT * NCLS)) { hulc_set_error("hulc_k_plan_gather: cb given: G=%d grow0=%d (need G >= 1 and grow0 past the %d plan rows)", G, grow0, NCAT * NCLS); return 1; }
    const int ta = t16 ? 2 : 4;
    if (k_misaligned(w_t, ta) || k_misaligned(idx, 4) || k_misaligned(b1, 4) || k_misaligned(b2, 4) || k_misaligned(out, 4) || k_misaligned(emb, ta) || k_misaligned(embg, ta) ||
        k_misaligned(goal, ta) || k_misaligned(cb, ta)) { hulc_set_error("hulc_k_plan_gather: a pointer is not aligned to its element type"); return 1; }
    if (NCAT > 0 && k_idx_out_of_range("hulc_k_plan_gather", idx, (long long)B * NCAT, NCLS, st)) return 1;
    if (!embg) { S = 0; W = 0; }
    HULC_K_T("hulc_k_plan_gather", launch_plan_gather<TT>(st, (const TT*)w_t, idx, B, NCAT, NCLS, H, b1, b2, out, (const TT*)emb, (TT*)embg, S, W, (const TT*)goal, G, grow0, (TT*)cb));
    return k_launched("hulc_k_plan_gather");
}

// form 0 = plan_scatter_grad_lds_kernel, 1 = plan_scatter_grad_w4_kernel (16-bit types only: plan_scatter_w4, the engine's own choice)
int k_plan_scatter_grad(int t16, int form, const void* dC, const int* idx, int B, int NCAT, int NCLS, int H, int KIN, float* dw, int store, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || NCAT < 1 || NCAT > 64 || NCLS < 1 || NCLS > 32 || H < 1 || KIN < NCAT * NCLS || (long long)B * H > (1ll << 30) || (long long)H * KIN > (1ll << 30)) {
        hulc_set_error("hulc_k_plan_scatter_grad: B=%d NCAT=%d NCLS=%d H=%d KIN=%d (need 1 <= NCAT <= 64, 1 <= NCLS <= 32: the LDS tile has 32 rows, KIN >= NCAT * NCLS)", B, NCAT, NCLS, H, KIN); return 1;
    }
    if (form != 0 && form != 1) { hulc_set_error("hulc_k_plan_scatter_grad: form must be 0 (lds) or 1 (w4), got %d", form); return 1; }
    if (store && form != 1) { hulc_set_error("hulc_k_plan_scatter_grad: store goes with form 1 (w4) only"); return 1; }
    if (store != 0 && store != 1) { hulc_set_error("hulc_k_plan_scatter_grad: store must be 0 or 1"); return 1; }
    if (!dC || !idx || !dw) { hulc_set_error("hulc_k_plan_scatter_grad: null argument"); return 1; }
    if (k_misaligned(dC, t16 ? 2 : 4) || k_misaligned(idx, 4) || k_misaligned(dw, 4)) { hulc_set_error("hulc_k_plan_scatter_grad: a pointer is not aligned to its element type"); return 1; }
    if (form == 1 && !(t16 ? plan_scatter_w4<h16_t>(NCLS) : plan_scatter_w4<float>(NCLS))) { hulc_set_error("hulc_k_plan_scatter_grad: form 1 (w4) serves the 16-bit types only"); return 1; }
    if (k_idx_out_of_range("hulc_k_plan_scatter_grad", idx, (long long)B * NCAT, NCLS, st)) return 1;
    HULC_K_T("hulc_k_plan_scatter_grad", launch_plan_scatter_grad<TT>(st, form == 1, (const TT*)dC, idx, B, NCAT, NCLS, H, KIN, dw, store));
    return k_launched("hulc_k_plan_scatter_grad");
}

int k_normal_kl_sample(int t16, const float* pr_state, const float* pp_state, int B, int n, const float* eps_in, float* eps_out, float* plan_f, void* plan_t, float* kl_elem,
                       float* dpp, float* dpr, float w_pp, float w_pr, unsigned long long seed, const float* lscale, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || n < 1 || (long long)B * n > (1ll << 29)) { hulc_set_error("hulc_k_normal_kl_sample: B=%d n=%d", B, n); return 1; }
    if (!pr_state || !eps_out || !plan_f || !plan_t || (pp_state && (!kl_elem || !dpp || !dpr))) { hulc_set_error("hulc_k_normal_kl_sample: null argument"); return 1; }
    if (k_misaligned(pr_state, 4) || k_misaligned(pp_state, 4) || k_misaligned(eps_in, 4) || k_misaligned(eps_out, 4) || k_misaligned(plan_f, 4) || k_misaligned(plan_t, t16 ? 2 : 4) ||
        k_misaligned(kl_elem, 4) || k_misaligned(dpp, 4) || k_misaligned(dpr, 4) || k_misaligned(lscale, 4)) { hulc_set_error("hulc_k_normal_kl_sample: a pointer is not aligned to its element type"); return 1; }
    HULC_K_T("hulc_k_normal_kl_sample", launch_normal_kl_sample<TT>(st, pr_state, pp_state, B, n, eps_in, eps_out, plan_f, (TT*)plan_t, kl_elem, dpp, dpr, w_pp, w_pr, seed, lscale));
    return k_launched("hulc_k_normal_kl_sample");
}

int k_normal_rsample_bwd(int t16, const float* dplan, const float* eps, const float* pr_state, const float* dpr_kl, int B, int n, void* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || n < 1 || (long long)B * n > (1ll << 29)) { hulc_set_error("hulc_k_normal_rsample_bwd: B=%d n=%d", B, n); return 1; }
    if (!dplan || !eps || !pr_state || !dpr_kl || !out) { hulc_set_error("hulc_k_normal_rsample_bwd: null argument"); return 1; }
    if (k_misaligned(dplan, 4) || k_misaligned(eps, 4) || k_misaligned(pr_state, 4) || k_misaligned(dpr_kl, 4) || k_misaligned(out, t16 ? 2 : 4)) {
        hulc_set_error("hulc_k_normal_rsample_bwd: a pointer is not aligned to its element type"); return 1;
    }
    HULC_K_T("hulc_k_normal_rsample_bwd", launch_normal_rsample_bwd<TT>(st, dplan, eps, pr_state, dpr_kl, B, n, (TT*)out));
    return k_launched("hulc_k_normal_rsample_bwd");
}

int k_layernorm_fwd(int t16, const float* x, long long ldx, int rows, int n, const float* g, const float* b, void* out, long long ldo, float* out_f32, long long ldf, float* stats,
                    void* stream) {
    if (rows < 1 || n < 1 || n > 128 || ldx < n || (out && ldo < n) || (out_f32 && ldf < n) || rows > (1 << 24)) {
        hulc_set_error("hulc_k_layernorm_fwd: rows=%d n=%d ldx=%lld ldo=%lld ldf=%lld (need 1 <= n <= 128 and leading dimensions >= n)", rows, n, ldx, ldo, ldf); return 1;
    }
    if (!x || !g || !b) { hulc_set_error("hulc_k_layernorm_fwd: null argument"); return 1; }
    if (k_misaligned(x, 4) || k_misaligned(g, 4) || k_misaligned(b, 4) || k_misaligned(out, t16 ? 2 : 4) || k_misaligned(out_f32, 4) || k_misaligned(stats, 4)) {
        hulc_set_error("hulc_k_layernorm_fwd: a pointer is not aligned to its element type"); return 1;
    }
    HULC_K_T("hulc_k_layernorm_fwd", launch_ln_fwd<TT>((hipStream_t)stream, x, ldx, rows, n, g, b, (TT*)out, ldo, out_f32, ldf, stats));
    return k_launched("hulc_k_layernorm_fwd");
}

// scratch: ln_bwd_scratch_floats(rows, n) floats for the fp32 pair (at most 2 * 64 * n), unused by the fused kernel
int k_layernorm_bwd(int t16, const float* dy, long long lddy, const float* x, long long ldx, const float* stats, const float* g, int rows, int n, float* dx_f32, long long ldd,
                    int accumulate, void* dx_t, long long ldt, float* dg, float* db, float drop_p, unsigned long long seed, int bcast_rows, float bcast_div, int dy_parts,
                    long long dy_part_stride, float* scratch, void* stream) {
    if (rows < 1 || n < 1 || n > 128 || lddy < n || ldx < n || (dx_f32 && ldd < n) || (dx_t && ldt < n) || rows > (1 << 24)) {
        hulc_set_error("hulc_k_layernorm_bwd: rows=%d n=%d lddy=%lld ldx=%lld ldd=%lld ldt=%lld (need 1 <= n <= 128 and leading dimensions >= n)", rows, n, lddy, ldx, ldd, ldt); return 1;
    }
    if (!dy || !x || !stats || !g || !dg || !db || (!dx_f32 && !dx_t)) { hulc_set_error("hulc_k_layernorm_bwd: null argument (dg, db and one of dx_f32, dx_t are required)"); return 1; }
    if (!(drop_p >= 0.f && drop_p < 1.f) || bcast_rows < 0 || dy_parts < 1 || dy_parts > 4 || (dy_parts > 1 && dy_part_stride < (long long)(rows - 1) * lddy + n) ||
        (bcast_rows > 0 && (!(bcast_div > 0.f) || rows % bcast_rows != 0))) {
        hulc_set_error("hulc_k_layernorm_bwd: drop_p=%g bcast_rows=%d bcast_div=%g dy_parts=%d dy_part_stride=%lld", (double)drop_p, bcast_rows, (double)bcast_div, dy_parts, dy_part_stride); return 1;
    }
    if (accumulate && !dx_f32) { hulc_set_error("hulc_k_layernorm_bwd: accumulate needs dx_f32"); return 1; }
    if (!t16 && (bcast_rows > 0 || dy_parts > 1)) { hulc_set_error("hulc_k_layernorm_bwd: fp32 runs the unfused pair, which has no bcast_rows / dy_parts (ln_bwd_can_bcast)"); return 1; }
    if (!t16 && !scratch) { hulc_set_error("hulc_k_layernorm_bwd: fp32 needs the scratch buffer of the parameter gradients"); return 1; }
    if (!t16 && drop_p > 0.f && !(dx_t && dx_f32)) { hulc_set_error("hulc_k_layernorm_bwd: fp32 masks dx_t as a copy of dx_f32: drop_p needs both"); return 1; }
    if (!t16 && (drop_p > 0.f || seed != 0) && dx_t && dx_f32 && (ldd != n || ldt != n)) { hulc_set_error("hulc_k_layernorm_bwd: fp32 with a dropout mask and both outputs needs ldd == ldt == n"); return 1; }
    if (k_misaligned(dy, 4) || k_misaligned(x, 4) || k_misaligned(stats, 4) || k_misaligned(g, 4) || k_misaligned(dx_f32, 4) || k_misaligned(dx_t, t16 ? 2 : 4) || k_misaligned(dg, 4) ||
        k_misaligned(db, 4) || k_misaligned(scratch, 4)) { hulc_set_error("hulc_k_layernorm_bwd: a pointer is not aligned to its element type"); return 1; }
    HULC_K_T("hulc_k_layernorm_bwd", launch_ln_bwd<TT>((hipStream_t)stream, scratch, dy, lddy, x, ldx, stats, g, rows, n, dx_f32, ldd, accumulate, (TT*)dx_t, ldt, dg, db, drop_p, seed,
              bcast_rows, bcast_div, dy_parts, dy_part_stride));
    return k_launched("hulc_k_layernorm_bwd");
}

int k_layernorm_mean(int t16, const float* x, int B, int S, int n, const float* g, const float* b, float* stats, void* out, float* yout, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || S < 1 || n < 1 || n > 128 || (long long)B * S * n > (1ll << 30)) { hulc_set_error("hulc_k_layernorm_mean: B=%d S=%d n=%d (need B, S >= 1 and 1 <= n <= 128)", B, S, n); return 1; }
    if (!x || !g || !b || !stats || !out || !yout) { hulc_set_error("hulc_k_layernorm_mean: null argument"); return 1; }
    if (k_misaligned(x, 4) || k_misaligned(g, 4) || k_misaligned(b, 4) || k_misaligned(stats, 4) || k_misaligned(out, t16 ? 2 : 4) || k_misaligned(yout, 4)) {
        hulc_set_error("hulc_k_layernorm_mean: a pointer is not aligned to its element type"); return 1;
    }
    HULC_K_T("hulc_k_layernorm_mean", launch_ln_mean<TT>(st, x, B, S, n, g, b, stats, (TT*)out, yout));
    return k_launched("hulc_k_layernorm_mean");
}
#undef HULC_K_T

// ---------------------------------------------------------------------------------------------------- fused transformer layer (tr_fused.h)
// The kernels read FRAGMENT-ORDERED weight copies (gemm.h: frag_pack_kernel).  The entries take plain row-major matrices, repack them into scratch exactly as
// Engine::prepare_weights does (one frag_pack_kernel launch over a FragPackBatch), launch through the engine's launch helper, and free the scratch after a stream synchronise.
struct KFragScratch {
    h16_t* base = nullptr;
    FragPackBatch fb{};
    int blocks = 0;
    size_t elems = 0, off[FRAG_PACK_MAX] = {};
    ~KFragScratch() { if (base) hipFree(base); }
    void add(const void* src, int N, int K) {      // N % 16 == 0, K % 128 == 0
        fb.src[fb.n] = (const h16_t*)src; off[fb.n] = elems; fb.N[fb.n] = N; fb.K[fb.n] = K; fb.blk0[fb.n] = blocks;
        blocks += frag_pack_blocks(N, K); elems += (size_t)N * K; ++fb.n; fb.blk0[fb.n] = blocks;
    }
    const h16_t* at(int i) const { return fb.dst[i]; }
    int alloc_and_pack(const char* who, hipStream_t st) {
        if (hipMalloc((void**)&base, elems * sizeof(h16_t)) != hipSuccess) { base = nullptr; hulc_set_error("%s: hipMalloc of the fragment-ordered weight copies failed", who); return 1; }
        for (int i = 0; i < fb.n; ++i) fb.dst[i] = base + off[i];
        hipLaunchKernelGGL(frag_pack_kernel, dim3(blocks), dim3(256), 0, st, fb);
        return k_launched(who);
    }
    int finish(const char* who, hipStream_t st) {
        if (k_launched(who)) return 1;
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { hulc_set_error("%s: %s", who, hipGetErrorString(e)); return 1; }
        return 0;
    }
};
static inline bool k_tr_shape_bad(const char* who, int B, int S, int smax, float dp) {
    if (B < 1 || S < 1 || S > smax || (long long)B * S > (1ll << 22)) { hulc_set_error("%s: B=%d S=%d (need B >= 1, 1 <= S <= %d, B * S <= 2^22)", who, B, S, smax); return true; }
    if (!(dp >= 0.f && dp < 1.f)) { hulc_set_error("%s: dp=%g outside [0, 1)", who, (double)dp); return true; }
    return false;
}

int k_tr_layer_fwd(const hulc_tr_layer_job* j, int B, int S, int ln_in, float dp, void* stream) {
    static const char* who = "hulc_k_tr_layer_fwd";
    hipStream_t st = (hipStream_t)stream;
    if (!j) { hulc_set_error("%s: null job", who); return 1; }
    if (k_tr_shape_bad(who, B, S, 64, dp)) return 1;
    if (ln_in != 0 && ln_in != 1) { hulc_set_error("%s: ln_in must be 0 or 1, got %d", who, ln_in); return 1; }
    if (!j->xin || !j->Wqkv || !j->Wo || !j->W1 || !j->W2 || !j->bqkv || !j->bo || !j->b1 || !j->b2 || !j->n1g || !j->n1b || !j->qkv || !j->Pat || !j->ao || !j->y1 || !j->st1 ||
        !j->x1t || !j->x1f || !j->hff || !j->y2) { hulc_set_error("%s: null pointer in the job", who); return 1; }
    if (ln_in && (!j->ln_g || !j->ln_b || !j->xf_out || !j->xt_out || !j->st_out)) { hulc_set_error("%s: ln_in = 1 needs ln_g, ln_b, xf_out, xt_out, st_out", who); return 1; }
    // 16-byte vectors: the weights (frag_pack_kernel), the four biases (f32x4), ao (u32x4), y1 (f32x4); 8-byte: qkv, hff (two packed pairs)
    if (k_misaligned16(j->Wqkv) || k_misaligned16(j->Wo) || k_misaligned16(j->W1) || k_misaligned16(j->W2) || k_misaligned16(j->bqkv) || k_misaligned16(j->bo) || k_misaligned16(j->b1) ||
        k_misaligned16(j->b2) || k_misaligned16(j->ao) || k_misaligned16(j->y1)) { hulc_set_error("%s: the weights, bqkv, bo, b1, b2, ao, y1 must be 16-byte aligned", who); return 1; }
    if (k_misaligned(j->qkv, 8) || k_misaligned(j->hff, 8)) { hulc_set_error("%s: qkv, hff must be 8-byte aligned", who); return 1; }
    if (k_misaligned(j->xin, 4) || k_misaligned(j->ln_g, 4) || k_misaligned(j->ln_b, 4) || k_misaligned(j->xf_out, 4) || k_misaligned(j->xt_out, 2) || k_misaligned(j->st_out, 4) ||
        k_misaligned(j->n1g, 4) || k_misaligned(j->n1b, 4) || k_misaligned(j->Pat, 4) || k_misaligned(j->st1, 4) || k_misaligned(j->x1t, 2) || k_misaligned(j->x1f, 4) ||
        k_misaligned(j->y2, 4)) { hulc_set_error("%s: a pointer is not aligned to its element type", who); return 1; }
    KFragScratch fs;
    fs.add(j->Wqkv, 3 * TRF_D, TRF_D); fs.add(j->Wo, TRF_D, TRF_D); fs.add(j->W1, TRF_FF, TRF_D); fs.add(j->W2, TRF_D, TRF_FF);
    if (fs.alloc_and_pack(who, st)) return 1;
    TrLayerP q{};
    q.xin = j->xin; q.ln_in = ln_in; q.ln_g = j->ln_g; q.ln_b = j->ln_b; q.xf_out = j->xf_out; q.xt_out = (h16_t*)j->xt_out; q.st_out = j->st_out;
    q.Wqkv = fs.at(0); q.Wo = fs.at(1); q.W1 = fs.at(2); q.W2 = fs.at(3);
    q.bqkv = j->bqkv; q.bo = j->bo; q.b1 = j->b1; q.b2 = j->b2; q.n1g = j->n1g; q.n1b = j->n1b;
    q.qkv = (h16_t*)j->qkv; q.Pat = j->Pat; q.ao = (h16_t*)j->ao; q.y1 = j->y1; q.st1 = j->st1; q.x1t = (h16_t*)j->x1t; q.x1f = j->x1f; q.hff = (h16_t*)j->hff; q.y2 = j->y2;
    q.B = B; q.S = S; q.dp = dp;
    q.seed_att = j->seed_att; q.seed_o = j->seed_o; q.seed_h = j->seed_h; q.seed_y = j->seed_y;
    launch_tr_layer_fwd(st, q);
    return fs.finish(who, st);
}

int k_tr_ffn_bwd(const hulc_tr_ffn_bwd_job* j, int B, int S, int bcast, float bdiv, float dp, void* stream) {
    static const char* who = "hulc_k_tr_ffn_bwd";
    hipStream_t st = (hipStream_t)stream;
    if (!j) { hulc_set_error("%s: null job", who); return 1; }
    if (k_tr_shape_bad(who, B, S, 64, dp)) return 1;
    if ((bcast != 0 && bcast != 1) || (bcast && !(bdiv > 0.f))) { hulc_set_error("%s: bcast=%d bdiv=%g (bcast is 0 or 1; with bcast, bdiv > 0)", who, bcast, (double)bdiv); return 1; }
    if (!j->dx || !j->y2 || !j->st2 || !j->n2g || !j->dg2 || !j->db2 || !j->W2t || !j->W1t || !j->hff || !j->dt_c || !j->dt_a || !j->part) { hulc_set_error("%s: null pointer in the job", who); return 1; }
    // 16-byte vectors: the weights (frag_pack_kernel), part (f32x4); 8-byte: hff, dt_a (two packed pairs)
    if (k_misaligned16(j->W2t) || k_misaligned16(j->W1t) || k_misaligned16(j->part)) { hulc_set_error("%s: W2t, W1t, part must be 16-byte aligned", who); return 1; }
    if (k_misaligned(j->hff, 8) || k_misaligned(j->dt_a, 8)) { hulc_set_error("%s: hff, dt_a must be 8-byte aligned", who); return 1; }
    if (k_misaligned(j->dx, 4) || k_misaligned(j->y2, 4) || k_misaligned(j->st2, 4) || k_misaligned(j->n2g, 4) || k_misaligned(j->dg2, 4) || k_misaligned(j->db2, 4) ||
        k_misaligned(j->dt_c, 2)) { hulc_set_error("%s: a pointer is not aligned to its element type", who); return 1; }
    KFragScratch fs;
    fs.add(j->W2t, TRF_FF, TRF_D); fs.add(j->W1t, TRF_D, TRF_FF);
    if (fs.alloc_and_pack(who, st)) return 1;
    TrFfnBwdP q{};
    q.dx = j->dx; q.bcast = bcast; q.bdiv = bdiv; q.y2 = j->y2; q.st2 = j->st2; q.n2g = j->n2g; q.dg2 = j->dg2; q.db2 = j->db2;
    q.W2t = fs.at(0); q.W1t = fs.at(1); q.hff = (const h16_t*)j->hff; q.dt_c = (h16_t*)j->dt_c; q.dt_a = (h16_t*)j->dt_a; q.part = j->part;
    q.B = B; q.S = S; q.N = (long long)B * S; q.dp = dp; q.seed_y = j->seed_y;
    launch_tr_ffn_bwd(st, q);
    return fs.finish(who, st);
}

int k_tr_attn_bwd(const hulc_tr_attn_bwd_job* j, int B, int S, int nparts, long long part_stride, float dp, void* stream) {
    static const char* who = "hulc_k_tr_attn_bwd";
    hipStream_t st = (hipStream_t)stream;
    if (!j) { hulc_set_error("%s: null job", who); return 1; }
    if (k_tr_shape_bad(who, B, S, 32, dp)) return 1;
    if (nparts < 1 || nparts > 4 || (nparts > 1 && part_stride < (long long)B * S * TRF_D)) {
        hulc_set_error("%s: nparts=%d part_stride=%lld (need 1 <= nparts <= 4 and, with more than one, part_stride >= B * S * 128)", who, nparts, part_stride); return 1;
    }
    if (!j->parts || !j->y1 || !j->st1 || !j->n1g || !j->dg1 || !j->db1 || !j->Wot || !j->Wint || !j->qkv || !j->Pat || !j->b_d || !j->b_b || !j->dy_f || !j->dx) {
        hulc_set_error("%s: null pointer in the job", who); return 1;
    }
    // 16-byte vectors: the weights (frag_pack_kernel), qkv (load8), b_b (Vec8 stores), dy_f (re-read as f32x4), dx (f32x4)
    if (k_misaligned16(j->Wot) || k_misaligned16(j->Wint) || k_misaligned16(j->qkv) || k_misaligned16(j->b_b) || k_misaligned16(j->dy_f) || k_misaligned16(j->dx)) {
        hulc_set_error("%s: Wot, Wint, qkv, b_b, dy_f, dx must be 16-byte aligned", who); return 1;
    }
    if (k_misaligned(j->parts, 4) || k_misaligned(j->y1, 4) || k_misaligned(j->st1, 4) || k_misaligned(j->n1g, 4) || k_misaligned(j->dg1, 4) || k_misaligned(j->db1, 4) ||
        k_misaligned(j->Pat, 4) || k_misaligned(j->b_d, 2)) { hulc_set_error("%s: a pointer is not aligned to its element type", who); return 1; }
    KFragScratch fs;
    fs.add(j->Wot, TRF_D, TRF_D); fs.add(j->Wint, TRF_D, 3 * TRF_D);
    if (fs.alloc_and_pack(who, st)) return 1;
    TrAttnBwdP q{};
    q.parts = j->parts; q.part_stride = part_stride; q.nparts = nparts; q.y1 = j->y1; q.st1 = j->st1; q.n1g = j->n1g; q.dg1 = j->dg1; q.db1 = j->db1;
    q.Wot = fs.at(0); q.Wint = fs.at(1); q.qkv = (const h16_t*)j->qkv; q.Pat = j->Pat; q.b_d = (h16_t*)j->b_d; q.b_b = (h16_t*)j->b_b; q.dy_f = j->dy_f; q.dx = j->dx;
    q.B = B; q.S = S; q.dp = dp; q.seed_o = j->seed_o; q.seed_att = j->seed_att;
    launch_tr_attn_bwd(st, q);
    return fs.finish(who, st);
}

// ---------------------------------------------------------------------------------------------------- the GEMM core with its runtime epilogue (gemm.h)
// hulc_k_gemm_epi / hulc_k_gemm_dual: a job mirrors EpiP field for field.  Everything is checked first — with the predicates the engine's routing uses (gemm_pick,
// gemm_glds_ok, skinny_ok, skinny_lds_kchunk_ok, skinny_lds_dual_ok) — and only then launched, through the launchers the engine calls.
// esz = bytes of the storage type T
static int k_gemm_job_bad(const char* who, int idx, const hulc_gemm_epi_job* jp, int esz) {
    if (!jp) { hulc_set_error("%s: null job", who); return 1; }
    const hulc_gemm_epi_job& j = *jp;
    if (!j.A || !j.B || !j.out) { hulc_set_error("%s: job %d: null pointer (A, B, out are required)", who, idx); return 1; }
    if (j.M < 1 || j.N < 1 || j.K < 1 || (long long)j.M * j.N > (1ll << 30) || j.lda < j.K || j.ldb < j.K || j.ldc < j.N) {
        hulc_set_error("%s: job %d: shape M=%d N=%d K=%d lda=%lld ldb=%lld ldc=%lld (need M, N, K >= 1, M * N <= 2^30, lda, ldb >= K, ldc >= N)", who, idx, j.M, j.N, j.K, (long long)j.lda,
                       (long long)j.ldb, (long long)j.ldc); return 1;
    }
    if ((j.out_s0 == 0) != (j.out_R1 == 0) || j.out_R1 < 0 || j.out_s0 < 0) {
        hulc_set_error("%s: job %d: output map out_R1=%d out_s0=%lld (both 0 = plain rows, or both > 0)", who, idx, j.out_R1, (long long)j.out_s0); return 1;
    }
    if (!(j.drop_p >= 0.f && j.drop_p < 1.f)) { hulc_set_error("%s: job %d: drop_p=%g outside [0, 1)", who, idx, (double)j.drop_p); return 1; }
    if (!(j.alpha == j.alpha) || j.alpha - j.alpha != 0.f) { hulc_set_error("%s: job %d: alpha is not finite", who, idx); return 1; }
    auto flag = [](int v) { return v == 0 || v == 1; };
    if (j.relu < 0 || j.relu > 2 || !flag(j.out_f32) || !flag(j.accumulate) || !flag(j.atomic) || !flag(j.res_f32) || !flag(j.res_late) || !flag(j.mask_tanh) || !flag(j.out2_relu) ||
        !flag(j.generic_only) || !flag(j.wfrag)) { hulc_set_error("%s: job %d: relu must be 0, 1 or 2 and every flag 0 or 1", who, idx); return 1; }
    if (j.res && (j.res_ld < j.N || j.res_rowmod < 0)) { hulc_set_error("%s: job %d: res_ld=%lld res_rowmod=%d (need res_ld >= N, res_rowmod >= 0)", who, idx, (long long)j.res_ld, j.res_rowmod); return 1; }
    if ((j.out2_lo & 3) || (j.out2_hi & 3) || j.out2_lo < 0 || j.out2_hi < j.out2_lo) {
        hulc_set_error("%s: job %d: out2_lo=%lld out2_hi=%lld must be multiples of 4 with 0 <= lo <= hi", who, idx, (long long)j.out2_lo, (long long)j.out2_hi); return 1;
    }
    if (j.out2 && (j.accumulate || j.atomic)) { hulc_set_error("%s: job %d: accumulate / atomic is never combined with out2", who, idx); return 1; }
    if (j.out2_mask && !j.out2) { hulc_set_error("%s: job %d: out2_mask without out2", who, idx); return 1; }
    if (j.atomic && !j.out_f32) { hulc_set_error("%s: job %d: atomic needs an fp32 output", who, idx); return 1; }
    if (j.nsplit < 1 || j.nsplit > 64 || j.z_stride < 0 || (j.z_stride & 3)) { hulc_set_error("%s: job %d: nsplit=%d z_stride=%lld (need 1 <= nsplit <= 64, z_stride >= 0 and a multiple of 4)", who, idx, j.nsplit, (long long)j.z_stride); return 1; }
    if (k_misaligned(j.A, esz) || k_misaligned(j.B, esz)) { hulc_set_error("%s: job %d: A, B are not aligned to their element type", who, idx); return 1; }
    if (k_misaligned16(j.bias) || k_misaligned16(j.bias2)) { hulc_set_error("%s: job %d: bias, bias2 must be 16-byte aligned (read as float4)", who, idx); return 1; }
    if (k_misaligned(j.out, 4 * (j.out_f32 ? 4 : esz)) || k_misaligned(j.res, 4 * (j.res_f32 ? 4 : esz)) || k_misaligned(j.mask, 4 * esz) || k_misaligned(j.out2, 4 * esz) ||
        k_misaligned(j.out2_mask, 4 * esz)) { hulc_set_error("%s: job %d: out, res, mask, out2, out2_mask must be aligned to four of their elements", who, idx); return 1; }
    return 0;
}
static EpiP k_gemm_job_epi(const hulc_gemm_epi_job& j) {
    EpiP e;
    e.out = j.out; e.out_f32 = j.out_f32; e.accumulate = j.accumulate; e.atomic = j.atomic; e.z_stride = j.z_stride; e.bias = j.bias; e.bias2 = j.bias2; e.res = j.res; e.res_f32 = j.res_f32;
    e.res_ld = j.res_ld; e.res_rowmod = j.res_rowmod; e.res_late = j.res_late; e.mask = j.mask; e.mask_tanh = j.mask_tanh; e.relu = j.relu; e.alpha = j.alpha; e.drop_p = j.drop_p;
    e.drop_seed = j.drop_seed; e.out2 = j.out2; e.out2_lo = j.out2_lo; e.out2_hi = j.out2_hi; e.out2_mask = j.out2_mask; e.out2_relu = j.out2_relu; e.generic_only = j.generic_only;
    return e;
}
static DenseOut k_gemm_job_om(const hulc_gemm_epi_job& j) { return j.out_s0 ? dense_out_map(j.out_R1, j.out_s0, j.ldc) : dense_out(j.ldc); }
// gemm_kernel at tile 32 / 64 / 128 with BK by the engine's rule (gemm_pick), nsplit K slabs
template <typename T>
static void k_gemm_tile(hipStream_t st, int tile, const DenseLoader<T>& a, const DenseLoader<T>& b, const DenseOut& om, const EpiP& ep, int M, int N, int K, int nsplit, bool bk32) {
    typedef DenseLoader<T> DL;
    if constexpr (sizeof(T) == 2) {
        if (K >= 128 && !bk32) {
            if (tile == 32) launch_gemm<T, 32, 32, DL, DL, DenseOut, 128>(st, a, b, om, ep, M, N, K, 1, nsplit);
            else if (tile == 64) launch_gemm<T, 64, 64, DL, DL, DenseOut, 128>(st, a, b, om, ep, M, N, K, 1, nsplit);
            else launch_gemm<T, 128, 128, DL, DL, DenseOut, 64>(st, a, b, om, ep, M, N, K, 1, nsplit);
            return;
        }
    }
    if (tile == 32) launch_gemm<T, 32, 32>(st, a, b, om, ep, M, N, K, 1, nsplit);
    else if (tile == 64) launch_gemm<T, 64, 64>(st, a, b, om, ep, M, N, K, 1, nsplit);
    else launch_gemm<T, 128, 128>(st, a, b, om, ep, M, N, K, 1, nsplit);
}
template <typename T>
static int k_gemm_epi_t(const hulc_gemm_epi_job& j, int kernel, int* ran, hipStream_t st) {
    static const char* who = "hulc_k_gemm_epi";
    const DenseLoader<T> a = dense<T>((const T*)j.A, j.M, j.lda), b = dense<T>((const T*)j.B, j.N, j.ldb);
    const DenseOut om = k_gemm_job_om(j);
    const EpiP ep = k_gemm_job_epi(j);
    const int M = j.M, N = j.N, K = j.K;
    if (kernel != 8 && j.atomic) { hulc_set_error("%s: atomic goes with kernel 8 (split K) only", who); return 1; }
    if (kernel != 7 && j.wfrag) { hulc_set_error("%s: wfrag goes with kernel 7 (the K-chunked kernel) only", who); return 1; }
    if ((kernel < 1 || kernel > 3) && kernel != 8 && (j.nsplit != 1 || j.z_stride != 0)) { hulc_set_error("%s: kernel %d takes nsplit = 1 and z_stride = 0", who, kernel); return 1; }
    if (kernel >= 1 && kernel <= 3 && (j.nsplit > 1) != (j.z_stride > 0)) { hulc_set_error("%s: kernels 1 .. 3: nsplit > 1 goes with z_stride > 0 (partial slabs) and the reverse", who); return 1; }
    if (kernel == 0) {
        const GemmPick pick = gemm_pick<T>(a, b, ep, M, N, K);
        if (!gemm_launch_picked<T>(st, pick, a, b, om, ep, M, N, K)) { hulc_set_error("%s: gemm_pick chose a kernel this type does not have", who); return 1; }
        *ran = pick == GEMM_PICK_SKINNY ? HULC_GEMM_RAN_SKINNY_ROUTER : pick == GEMM_PICK_GLDS ? HULC_GEMM_RAN_GLDS : gemm_pick_tile(pick) == 128 ? HULC_GEMM_RAN_128 :
               gemm_pick_tile(pick) == 64 ? HULC_GEMM_RAN_64 : HULC_GEMM_RAN_32;
        return k_launched(who);
    }
    if (kernel >= 1 && kernel <= 3) {
        k_gemm_tile<T>(st, 16 << kernel, a, b, om, ep, M, N, K, j.nsplit, false);
        *ran = kernel;
        return k_launched(who);
    }
    if (kernel == 8) {
        if (!j.atomic || !j.out_f32 || j.nsplit < 2 || j.z_stride != 0) { hulc_set_error("%s: kernel 8 (split K) needs atomic = 1, out_f32 = 1, nsplit >= 2, z_stride = 0", who); return 1; }
        bool big = false;
        gemm_wgrad_nsplit<T>(M, N, K, &big);
        k_gemm_tile<T>(st, big ? 128 : 64, a, b, om, ep, M, N, K, j.nsplit, true);      // Engine::gemm_wgrad: BK = 32
        *ran = big ? HULC_GEMM_RAN_SPLITK_128 : HULC_GEMM_RAN_SPLITK_64;
        return k_launched(who);
    }
    if constexpr (sizeof(T) == 2) {
        const h16_t* A = (const h16_t*)j.A; const h16_t* W = (const h16_t*)j.B;
        if (kernel == 4) {
            if (!gemm_glds_ok(a, b, ep, M, N, K)) { hulc_set_error("%s: kernel 4: gemm_glds_ok refuses (K >= 64, K %% 32 == 0, rows 16-byte aligned, z_stride 0)", who); return 1; }
            launch_gemm_glds(st, a, b, om, ep, M, N, K);
            *ran = HULC_GEMM_RAN_GLDS;
            return k_launched(who);
        }
        if (kernel >= 5 && kernel <= 7 && !skinny_ok(M, N, K, j.lda, j.ldb, A, W)) {
            hulc_set_error("%s: kernel %d: skinny_ok refuses (M <= 64 or few rows of tiles, K %% 32 == 0, K >= 128, N %% 16 == 0, rows 16-byte aligned)", who, kernel); return 1;
        }
        if (kernel == 5 || kernel == 6) {
            launch_skinny(st, A, j.lda, W, j.ldb, M, N, K, om, ep, kernel == 5);
            *ran = kernel;
            return k_launched(who);
        }
        if (kernel == 7) {
            if (!skinny_lds_kchunk_ok(A, j.lda, M, N, K)) { hulc_set_error("%s: kernel 7: shape not covered by the K-chunked kernel (K = n x 2048 > 2048, M <= 64, lda %% 64 == 0, A 128-byte aligned)", who); return 1; }
            if (j.wfrag && (j.ldb != K || k_misaligned16(W))) { hulc_set_error("%s: kernel 7: wfrag repacks a dense B (ldb == K, 16-byte aligned)", who); return 1; }
            KFragScratch fs;
            if (j.wfrag) { fs.add(W, N, K); if (fs.alloc_and_pack(who, st)) return 1; }
            if (!launch_skinny_lds_kchunk(st, A, j.lda, j.wfrag ? fs.at(0) : W, j.wfrag ? 0ll : (long long)j.ldb, M, N, K, om, ep)) { hulc_set_error("%s: kernel 7: the launcher refused", who); return 1; }
            *ran = HULC_GEMM_RAN_KCHUNK;
            return j.wfrag ? fs.finish(who, st) : k_launched(who);
        }
    }
    hulc_set_error("%s: kernel %d is unknown, or a 16-bit kernel asked of fp32", who, kernel);
    return 1;
}
// t16: 0 = float, 1 = this translation unit's 16-bit type
int k_gemm_epi(int t16, const hulc_gemm_epi_job* j, int kernel, int* ran, void* stream) {
    int dummy = 0;
    if (!ran) ran = &dummy;
    *ran = HULC_GEMM_RAN_NONE;
    if (k_gemm_job_bad("hulc_k_gemm_epi", 0, j, t16 ? 2 : 4)) return 1;
    if (t16) return k_gemm_epi_t<h16_t>(*j, kernel, ran, (hipStream_t)stream);
#ifdef HULC_HALF_F16
    hulc_set_error("hulc_k_gemm_epi: the fp32 instances live in the bf16 translation unit"); return 1;
#else
    return k_gemm_epi_t<float>(*j, kernel, ran, (hipStream_t)stream);
#endif
}
// two independent recurrent steps of one shape as ONE launch (launch_skinny_lds_dual): jobs[0] and jobs[1]
int k_gemm_dual(const hulc_gemm_epi_job* jobs, int* ran, void* stream) {
    static const char* who = "hulc_k_gemm_dual";
    hipStream_t st = (hipStream_t)stream;
    int dummy = 0;
    if (!ran) ran = &dummy;
    *ran = HULC_GEMM_RAN_NONE;
    if (!jobs) { hulc_set_error("%s: null jobs", who); return 1; }
    DenseLoader<h16_t> a[2], b[2]; DenseOut om[2]; EpiP ep[2];
    for (int i = 0; i < 2; ++i) {
        const hulc_gemm_epi_job& j = jobs[i];
        if (k_gemm_job_bad(who, i, &j, 2)) return 1;
        if (j.nsplit != 1 || j.z_stride != 0 || j.atomic || j.wfrag) { hulc_set_error("%s: job %d: nsplit = 1, z_stride = 0, no atomic, no wfrag", who, i); return 1; }
        a[i] = dense<h16_t>((const h16_t*)j.A, j.M, j.lda); b[i] = dense<h16_t>((const h16_t*)j.B, j.N, j.ldb); om[i] = k_gemm_job_om(j); ep[i] = k_gemm_job_epi(j);
    }
    const hulc_gemm_epi_job &j0 = jobs[0], &j1 = jobs[1];
    if (j0.M != j1.M || j0.N != j1.N || j0.K != j1.K || j0.lda != j1.lda || j0.ldb != j1.ldb || j0.ldc != j1.ldc || j0.out_R1 != j1.out_R1 || j0.out_s0 != j1.out_s0) {
        hulc_set_error("%s: the two jobs share M, N, K, the leading dimensions and the output map", who); return 1;
    }
    if (!skinny_lds_dual_ok(a[0].p, b[0].p, a[1].p, b[1].p, j0.lda, j0.ldb, j0.M, j0.N, j0.K)) {
        hulc_set_error("%s: shape not covered by the dual launch (32 < M <= 64, K = 2048, N %% 16 == 0, lda %% 64 == 0, A 128-byte aligned, W 16-byte aligned)", who); return 1;
    }
    if (!launch_skinny_lds_dual(st, a[0].p, b[0].p, ep[0], a[1].p, b[1].p, ep[1], j0.lda, j0.ldb, j0.M, j0.N, j0.K, om[0])) { hulc_set_error("%s: the launcher refused", who); return 1; }
    *ran = HULC_GEMM_RAN_DUAL;
    return k_launched(who);
}
// host arithmetic only: the routing functions of gemm.h behind a C entry (tests/test_gemm_epi_ref_host.py)
int k_gemm_pick(int t16, int M, int N, int K, long long lda, long long ldb, int* pick, int* bk) {
    if (!pick || !bk || M < 1 || N < 1 || K < 1 || lda < K || ldb < K) { hulc_set_error("hulc_k_gemm_pick: null argument or bad shape"); return 1; }
    EpiP ep;
    GemmPick p;
    const void* al = (const void*)(uintptr_t)0x10000;       // never dereferenced: stands for an aligned operand
    if (t16) p = gemm_pick<h16_t>(dense<h16_t>((const h16_t*)al, M, lda), dense<h16_t>((const h16_t*)al, N, ldb), ep, M, N, K);
    else p = gemm_pick<float>(dense<float>((const float*)al, M, lda), dense<float>((const float*)al, N, ldb), ep, M, N, K);
    *pick = p == GEMM_PICK_SKINNY ? HULC_GEMM_RAN_SKINNY_ROUTER : p == GEMM_PICK_GLDS ? HULC_GEMM_RAN_GLDS : gemm_pick_tile(p) == 128 ? HULC_GEMM_RAN_128 : gemm_pick_tile(p) == 64 ? HULC_GEMM_RAN_64 : HULC_GEMM_RAN_32;
    *bk = (p == GEMM_PICK_SKINNY || p == GEMM_PICK_GLDS) ? 0 : (p == GEMM_PICK_64_BK128 || p == GEMM_PICK_32_BK128) ? 128 : p == GEMM_PICK_128_BK64 ? 64 : 32;
    return 0;
}
int k_gemm_wgrad_nsplit(int t16, int M, int N, int K, int* nsplit, int* big) {
    if (!nsplit || !big || M < 1 || N < 1 || K < 1) { hulc_set_error("hulc_k_gemm_wgrad_nsplit: null argument or bad shape"); return 1; }
    bool b = false;
    *nsplit = t16 ? gemm_wgrad_nsplit<h16_t>(M, N, K, &b) : gemm_wgrad_nsplit<float>(M, N, K, &b);
    *big = b ? 1 : 0;
    return 0;
}

// hulc_k_lin_bwd_stream: lin_bwd_stream_kernel (lin_bwd.h) on one job, rows split into nsplit ranges; the four forms the engine launches.  slabs == null, nsplit = 1: the
// tile is stored to (store != 0) or added to dW by the kernel itself; slabs == null, nsplit > 1: the ranges add to dW with fp32 atomics (store != 0: dW is cleared first).
// slabs given (any nsplit, 1 included: the decoder heads' form): every range stores its slab ([nsplit][N][K], never read before it is written) and slab_sum_kernel
// adds them to dW in index order (store != 0: dW is cleared first).  nsplit > 1: the bias sums of the ranges land in db with atomics.  db (may be null) is always added to.
int k_lin_bwd_stream(const void* dY, const void* X, long long ldx, int M, int N, int K, int nsplit, int store, float* dW, long long lddw, float* db, float* slabs, void* stream) {
    static const char* who = "hulc_k_lin_bwd_stream";
    hipStream_t st = (hipStream_t)stream;
    if (!dY || !X || !dW || M < 1 || N < 1 || K < 1 || ldx < K || lddw < K || nsplit < 1 || nsplit > 64) { hulc_set_error("%s: null argument or bad shape (M=%d N=%d K=%d nsplit=%d)", who, M, N, K, nsplit); return 1; }
    if ((long long)M * std::max<long long>(N, ldx) >= (1ll << 31) || (long long)N * lddw >= (1ll << 31)) { hulc_set_error("%s: operand too large", who); return 1; }
    if (!lin_stream_ok(dY, X, ldx, N)) { hulc_set_error("%s: rows must start 8-byte aligned (N, ldx multiples of 4; dY, X 8-byte aligned)", who); return 1; }
    if (k_misaligned16(slabs)) { hulc_set_error("%s: the slab buffer [nsplit][N][K] must be 16-byte aligned", who); return 1; }
    LinStreamBatch bt{};
    int blocks = 0;
    lin_stream_add(bt, blocks, (const h16_t*)dY, (const h16_t*)X, ldx, M, N, K, dW, lddw, db, slabs, nsplit, store ? 1 : 0);
    const bool clear = store && (slabs || nsplit > 1);      // the slab sum and the atomics add
    if (clear && hipMemset2DAsync(dW, sizeof(float) * lddw, 0, sizeof(float) * K, N, st) != hipSuccess) { hulc_set_error("%s: clearing dW failed", who); return 1; }
    launch_lin_stream(st, bt, blocks);
    if (slabs) {
        const int vec = (K & 3) == 0 && (lddw & 3) == 0 && !k_misaligned16(dW);
        hipLaunchKernelGGL(slab_sum_kernel, dim3(cdiv((long long)N * K, vec ? 1024 : 256)), dim3(256), 0, st, (const float*)slabs, nsplit, (long long)N * K, N, K, dW, lddw, vec);
    }
    return k_launched(who);
}

// ---------------------------------------------------------------------------------------------------- the encoder's convolution family (conv_tile.h, conv_reg.h, conv_wgrad.h, conv1_wgrad.h)
// hulc_k_conv_wgrad, hulc_k_conv1_wgrad_u8, hulc_k_conv_tile, hulc_k_conv_pair (the bf16 wrappers: typed == 0) and their per-type forms hulc_k_*_t (typed == 1), launched
// through the launchers engine_encoders.inc calls.  who = the C entry's name (error messages).  typed: the bench-only forms no launch site of engine_encoders.inc names
// are refused — the 8-wave data-gradient forms (modes 12 / 13 / 18 / 19), the register-staged uint8 conv1 forward (relu bit 256) and the uint8 conv1 weight-gradient
// form 1 — and out_side must belong to in_side and a data-gradient form must come with its mask; the fp16 unit does not instantiate the 8-wave data-gradient kernels at all.
// slabs (may be null): the number of partial slabs that were summed into the weight gradient (the pair entry: two numbers)
static inline int k_conv_fwd_side(int in_side, int K, int S) { return in_side < K ? -1 : (in_side - K) / S + 1; }
static inline bool k_conv_mode_bench_only(int mode) { return mode == 12 || mode == 13 || mode == 18 || mode == 19; }
// which = 1: conv1 from fp32 NCHW frames, out [32][192] in (c,kh,kw) order; 2 / 3: conv2 / conv3 from 16-bit NHWC, out [64][KH*KW*CI] in packed (kh,kw,ci) order
int k_conv_wgrad(const char* who, int typed, int which, const void* X, const void* dY, float* out, float* db_out, int Nf, int IH, int* slabs, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (slabs) *slabs = 0;
    if (typed) {      // every argument is checked before anything is allocated or launched
        if (which < 1 || which > 3) { hulc_set_error("%s: which must be 1, 2 or 3", who); return 1; }
        const int KH = which == 3 ? 3 : (which == 2 ? 4 : 8);
        if (!X || !dY || !out || Nf < 1 || IH < KH || IH > 4096 || (long long)Nf * IH * IH * 64 >= (1ll << 31)) { hulc_set_error("%s: null argument, or Nf=%d, IH=%d out of range", who, Nf, IH); return 1; }
    }
    float* part = nullptr;
    static float* bias_tmp = nullptr;
    if (!bias_tmp && hipMalloc(&bias_tmp, sizeof(float) * 512 * 64) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
    const int KC = which == 3 ? 576 : (which == 2 ? 512 : 192);
    const int CO = which == 1 ? 32 : 64;
    if (hipMalloc(&part, sizeof(float) * 512ll * 64 * KC) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
    int ns;
    static h16_t* zp = nullptr;                   // zero page of the LDS-DMA kernel (pad slots, columns / rows beyond the frame)
    if (!zp) { if (hipMalloc(&zp, 256) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; } hipMemset(zp, 0, 256); }
    if (db_out) hipMemsetAsync(bias_tmp, 0, sizeof(float) * 64, st);      // the kernels add their bias partials to bias_tmp[0 .. CO)
    WgradJob J{}; J.X = (const h16_t*)X; J.dY = (const h16_t*)dY; J.part = part; J.bias_part = bias_tmp; J.zeros = zp; J.Nf = Nf; J.IH = J.IW = IH; J.FPB = 1;
    if (which == 3) { J.OH = J.OW = IH - 2; ns = launch_conv_wgrad_tr<64, 64, 3, 3, 1>(st, J, 512); }
    else if (which == 2) { J.OH = J.OW = (IH - 4) / 2 + 1; ns = launch_conv_wgrad_tr<32, 64, 4, 4, 2>(st, J, 512); }
    else if (which == 1) { const int OH = (IH - 8) / 4 + 1; ns = launch_conv1_wgrad_tr(st, Conv1Src{X, nullptr, 0, 0}, (const h16_t*)dY, part, bias_tmp, Nf, IH, IH, OH, OH, 512); }
    else { hipFree(part); hulc_set_error("%s: which must be 1, 2 or 3", who); return 1; }
    hipMemsetAsync(out, 0, sizeof(float) * CO * KC, st);
    hipLaunchKernelGGL(unpack_conv_wgrad_kernel, dim3((CO * KC + 1023) / 1024), dim3(256), 0, st, part, ns, (long long)CO * KC, out, CO, KC, 1, 1, 0);
    if (db_out) hipMemcpyAsync(db_out, bias_tmp, sizeof(float) * CO, hipMemcpyDeviceToDevice, st);
    hipError_t e = hipStreamSynchronize(st);
    hipFree(part);
    if (e != hipSuccess) { hulc_set_error("%s: %s", who, hipGetErrorString(e)); return 1; }
    if (slabs) *slabs = ns;
    return 0;
}

// conv1's weight gradient from uint8 (Nf,IH,IH,3) frames alone: dW (32,192) [torch (o, c, kh, kw) order] and db (32) of the frames after ScaleImageTensor / Normalize /
// RandomShiftsAug — form 1: conversion from the prefetch registers (conv1_wgrad_tr2r_kernel), 2: the same with interior / row-end slots (the engine's); fold = Conv1Src::fold
int k_conv1_wgrad_u8(const char* who, int typed, const void* X, const int* shifts, int pad, const void* dY, float* dw_out, float* db_out, int Nf, int IH, int form, int fold, int* slabs,
                     void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (slabs) *slabs = 0;
    if (form != 1 && form != 2) { hulc_set_error("%s: form must be 1 or 2 (got %d)", who, form); return 1; }      // before any device call
    if (typed) {
        if (form != 2) { hulc_set_error("%s: form %d is a bench-only form (the engine runs form 2)", who, form); return 1; }
        if (!X || !dY || !dw_out || !db_out || Nf < 1 || IH < 8 || IH > 4096 || pad < 0 || pad > CONV1_RAW_MARGIN) { hulc_set_error("%s: null argument, or Nf=%d, IH=%d, pad=%d out of range", who, Nf, IH, pad); return 1; }
    }
    float *part = nullptr, *bias = nullptr;
    if (hipMalloc(&part, sizeof(float) * 512ll * 32 * 192) != hipSuccess || hipMalloc(&bias, sizeof(float) * 64) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
    hipMemsetAsync(bias, 0, sizeof(float) * 64, st);
    Conv1Src src{}; src.X = X; src.shift = shifts; src.u8 = 1; src.pad = pad; src.fold = fold != 0;
    const int OH = (IH - 8) / 4 + 1;
    const int ns = launch_conv1_wgrad_tr(st, src, (const h16_t*)dY, part, bias, Nf, IH, IH, OH, OH, 512, nullptr, form);
    hipMemsetAsync(dw_out, 0, sizeof(float) * 32 * 192, st);
    hipLaunchKernelGGL(unpack_conv_wgrad_kernel, dim3((32 * 192 + 1023) / 1024), dim3(256), 0, st, part, ns, (long long)32 * 192, dw_out, 32, 192, 1, 1, 0);
    hipMemcpyAsync(db_out, bias, sizeof(float) * 32, hipMemcpyDeviceToDevice, st);
    hipError_t e = hipStreamSynchronize(st);
    hipFree(part); hipFree(bias);
    if (e != hipSuccess) { hulc_set_error("%s: %s", who, hipGetErrorString(e)); return 1; }
    if (slabs) *slabs = ns;
    return 0;
}

// raw-tile / weights-in-registers conv kernels alone (16-bit NHWC): the modes of include/hulc_hip.h.  bits1_out (typed, modes 4 .. 6): conv1's ReLU bit words, one per pixel
// wgs (typed, the weights-in-registers modes 10 .. 29): the persistent workgroups of the launch (several items per workgroup, stacks sized for them); 0 = the launcher's own
int k_conv_tile(const char* who, int typed, int mode, const void* img, const void* w, const float* bias, const void* mask, void* out, unsigned* bits1_out, int Nf, int IMH, int OUTH,
                int relu, int wgs, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    // every argument is checked before anything is allocated or launched.  relu: bit 0 = ReLU, bit 5 (32) = dynamic work claiming, bit 8 (256, modes 5 / 6) = the
    // register-staged uint8 conv1 forward (conv1_fwd_kernel<4, true>, the cross-check of the LDS-DMA kernel)
    if (mode < 0 || mode > 29 || (mode >= 14 && mode <= 16) || (mode >= 24 && mode <= 26)) { hulc_set_error("%s: unsupported mode %d", who, mode); return 1; }
    if ((relu & ~(1 | 32 | 256)) || ((relu & 256) && mode != 5 && mode != 6)) { hulc_set_error("%s: unknown bits in relu (%d) for mode %d", who, relu, mode); return 1; }
#ifdef HULC_HALF_F16
    if (k_conv_mode_bench_only(mode)) { hulc_set_error("%s: mode %d is a bench-only form: bf16 only", who, mode); return 1; }
#endif
    if (typed) {
        if (k_conv_mode_bench_only(mode) || (relu & 256)) { hulc_set_error("%s: mode %d, relu %d is a bench-only form no launch site of the engine names", who, mode, relu); return 1; }
        const int m10 = mode % 10;
        const bool c1 = mode >= 4 && mode <= 6, dg = !c1 && (m10 == 2 || m10 == 3 || m10 == 8 || m10 == 9), k3 = !c1 && (m10 == 0 || m10 == 2 || m10 == 8);
        if (!img || !w || !out || (!dg && !bias) || Nf < 1 || IMH < 1 || OUTH < 1 || IMH > 4096 || OUTH > 4096) { hulc_set_error("%s: null argument, or Nf=%d, IMH=%d, OUTH=%d out of range", who, Nf, IMH, OUTH); return 1; }
        const int want = c1 ? k_conv_fwd_side(IMH, 8, 4) : (k3 ? k_conv_fwd_side(dg ? OUTH : IMH, 3, 1) : k_conv_fwd_side(dg ? OUTH : IMH, 4, 2));
        if (want < 1 || want != (dg ? IMH : OUTH)) { hulc_set_error("%s: mode %d: out_side %d does not belong to in_side %d", who, mode, OUTH, IMH); return 1; }
        if (dg && !mask) { hulc_set_error("%s: mode %d is a data-gradient form and needs its mask", who, mode); return 1; }
        if (mode == 6 && !mask) { hulc_set_error("%s: mode 6 needs the shifts in mask", who); return 1; }
        if (!c1 && !dg && !(relu & 1)) { hulc_set_error("%s: mode %d: the forward forms run with ReLU (relu bit 0)", who, mode); return 1; }
        if (wgs < 0 || wgs > 512 || (wgs && mode < 10)) { hulc_set_error("%s: wgs=%d (0 .. 512; the weights-in-registers modes 10 .. 29 only)", who, wgs); return 1; }
        if (bits1_out && !c1) { hulc_set_error("%s: bits1_out goes with the conv1 forward (modes 4 .. 6); the conv2 forms emit their bit words into mask", who); return 1; }
    }
    ConvTileP p{}; p.img = (const h16_t*)img; p.IMH = p.IMW = IMH; p.w = (const h16_t*)w; p.out = (h16_t*)out; p.OUTH = p.OUTW = OUTH;
    p.bias = bias; p.mask = (const h16_t*)mask; p.relu = relu & 1; p.Nf = Nf;
    // modes 7..9 = the production forms: 7 = mode 1 that also EMITS the ReLU bitmask of its output into `mask` (unsigned[Nf][OUTH][OUTW][2]);
    // 8 / 9 = modes 2 / 3 with `mask` = ReLU bitmask words (2 / 1 per output pixel) staged through LDS.  relu bit 5 (32): dynamic work claiming.
    if (mode == 7) { p.mask = nullptr; p.bits_out = (unsigned*)mask; mode = 1; }
    else if (mode == 8 || mode == 9) { p.mask = nullptr; p.maskbits = (const unsigned*)mask; mode -= 6; }
    if (relu & 32) {
        static int* ctr = nullptr;
        if (!ctr && hipMalloc(&ctr, 256) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
        hipMemsetAsync(ctr, 0, 256, st);
        p.work_ctr = ctr;
    }
    {   // conv_reg.h pipelined-epilogue forms (modes 28 / 29 and what falls back from them): a scratch page for the stores of pixels that must not be written
        static void* dp = nullptr;
        if (!dp && hipMalloc(&dp, 8192) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
        p.dump = (h16_t*)dp;
    }
    bool ok = false;
    const int* const wgp = (typed && wgs > 0) ? &wgs : nullptr;
    // modes 10 / 11 / 17: modes 0 / 1 / 7 on the weights-in-registers kernels (conv_reg.h); 12 / 18: modes 2 / 8 (conv3 data gradient, 16-bit mask / bitmask)
    if (mode == 17) { p.mask = nullptr; p.bits_out = (unsigned*)mask; mode = 11; }
    if (mode == 18) { p.mask = nullptr; p.maskbits = (const unsigned*)mask; mode = 12; }
    if (mode == 19) { p.mask = nullptr; p.maskbits = (const unsigned*)mask; mode = 13; }      // 13 / 19: modes 3 / 9 (conv2 data gradient, four parity classes)
    // modes 20 / 21 / 27 / 22 / 28 / 23 / 29: modes 10 .. 19 in the form with two 256-thread workgroups per CU (conv_reg.h, NWV = 4)
    if (mode == 27) { p.mask = nullptr; p.bits_out = (unsigned*)mask; mode = 21; }
    if (mode == 28) { p.mask = nullptr; p.maskbits = (const unsigned*)mask; mode = 22; }
    if (mode == 29) { p.mask = nullptr; p.maskbits = (const unsigned*)mask; mode = 23; }
    if (mode == 12 || mode == 13 || mode == 22 || mode == 23) {      // the data-gradient forms stage their zero border from a zero page
        static void* zp = nullptr;
        if (!zp) { if (hipMalloc(&zp, 256) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; } hipMemset(zp, 0, 256); }
        p.zeros = (const h16_t*)zp;
    }
    if (mode == 20) ok = launch_conv_reg_jobs<64, 3, 3, 1, false, 1, 4>(st, &p, 1, wgp);
    else if (mode == 21) ok = launch_conv_reg_jobs<32, 4, 4, 2, false, 1, 4, true>(st, &p, 1, wgp);         // the production form for small maps: slot decode in registers (conv_reg.h PKR)
    else if (mode == 22) ok = launch_conv_reg_jobs<64, 3, 3, 1, true, 1, 4, true, 1>(st, &p, 1, wgp);       // the production forms: PKR + pipelined epilogue (EPI; 16-bit mask values
    else if (mode == 23) ok = launch_conv_reg_jobs<64, 2, 2, 1, true, 2, 4, true, 1>(st, &p, 1, wgp);       // = modes 22 / 23 fall back to the pair form inside launch_conv_reg)
    else if (mode == 10) ok = launch_conv_reg_fwd_jobs<64, 3, 3, 1>(st, &p, 1, wgp);
    else if (mode == 11) ok = launch_conv_reg_fwd_jobs<32, 4, 4, 2>(st, &p, 1, wgp);
#ifndef HULC_HALF_F16
    else if (mode == 12) ok = launch_conv_reg<64, 3, 3, 1, true>(st, p);
    else if (mode == 13) ok = launch_conv_reg<64, 2, 2, 1, true, 2>(st, p);
#endif
    else if (mode == 0) ok = launch_conv_tile<64, 64, 3, 3, 1, 1, false>(st, p);
    else if (mode == 1) ok = launch_conv_tile<32, 64, 4, 4, 2, 1, false>(st, p);
    else if (mode == 2) ok = launch_conv_tile<64, 64, 3, 3, 1, 1, true>(st, p);
    else if (mode == 3) ok = launch_conv_tile<64, 32, 2, 2, 1, 2, true>(st, p);
    else if (mode == 4) { launch_conv1_fwd(st, Conv1Src{img, nullptr, 0, 0}, (const h16_t*)w, bias, (h16_t*)out, Nf, IMH, IMH, OUTH, OUTH, false, bits1_out); ok = true; }
    else if (mode == 5 || mode == 6) {      // conv1 forward from uint8 NHWC frames; mode 6: `mask` = (Nf,2) int32 RandomShiftsAug shifts, pad 10 (IMH >= 100) or 4
        launch_conv1_fwd(st, Conv1Src{img, mode == 6 ? (const int*)mask : nullptr, 1, IMH >= 100 ? 10 : 4}, (const h16_t*)w, bias, (h16_t*)out, Nf, IMH, IMH, OUTH,
                         OUTH, (relu & 256) != 0, bits1_out);
        ok = true;
    }
    if (!ok) { hulc_set_error("%s: unsupported mode/shape", who); return 1; }
    if (hipGetLastError() != hipSuccess) { hulc_set_error("%s: launch failed", who); return 1; }
    return 0;
}

// One stage of both encoders as ONE launch (conv_reg.h launch_conv_reg_jobs, conv_wgrad.h launch_conv_wgrad_pair /
// conv1_wgrad.h launch_conv1_wgrad_jobs) in the forms the engine runs, dynamic claiming on (one zeroed counter per job, as the engine's next_ctr()); b == NULL: job a alone through the same entry
int k_conv_pair(const char* who, int typed, int stage, const hulc_conv_job* a, const hulc_conv_job* b, int wg_a, int wg_b, int* slabs, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const bool fwd = stage == HULC_PAIR_CONV2_FWD || stage == HULC_PAIR_CONV3_FWD, dgr = stage == HULC_PAIR_CONV3_DGRAD || stage == HULC_PAIR_CONV2_DGRAD;
    const bool wgr = stage == HULC_PAIR_CONV3_WGRAD || stage == HULC_PAIR_CONV2_WGRAD || stage == HULC_PAIR_CONV1_WGRAD;
    if (slabs) slabs[0] = slabs[1] = 0;
    // every argument is checked before anything is allocated or written
    if (!fwd && !dgr && !wgr) { hulc_set_error("%s: unknown stage %d", who, stage); return 1; }
    if (!a) { hulc_set_error("%s: job a is required", who); return 1; }
    if (wg_a < 1 || (b && wg_b < 1)) { hulc_set_error("%s: every job needs at least one workgroup", who); return 1; }
    if (wgr && !b) { hulc_set_error("%s: the weight-gradient stages need both jobs", who); return 1; }
    {
        const hulc_conv_job* src[2] = {a, b};
        for (int k = 0; k < (b ? 2 : 1); ++k)
            if (!src[k]->in || !src[k]->w || !src[k]->out || src[k]->frames < 1 || src[k]->in_side < 1 || src[k]->out_side < 1 || (wgr && !src[k]->bits)) { hulc_set_error("%s: incomplete job", who); return 1; }
    }
    if (wgr) {
        const int KH = stage == HULC_PAIR_CONV1_WGRAD ? 8 : (stage == HULC_PAIR_CONV3_WGRAD ? 3 : 4), S = stage == HULC_PAIR_CONV1_WGRAD ? 4 : (stage == HULC_PAIR_CONV3_WGRAD ? 1 : 2);
        if (a->in_side < KH || b->in_side < KH || a->out_side != (a->in_side - KH) / S + 1 || b->out_side != (b->in_side - KH) / S + 1) { hulc_set_error("%s: out_side does not belong to in_side", who); return 1; }
    } else if (typed) {
        const bool k3 = stage == HULC_PAIR_CONV3_FWD || stage == HULC_PAIR_CONV3_DGRAD;
        const hulc_conv_job* src[2] = {a, b};
        for (int k = 0; k < (b ? 2 : 1); ++k) {
            const int big = dgr ? src[k]->out_side : src[k]->in_side, small = dgr ? src[k]->in_side : src[k]->out_side;
            if (big > 4096 || k_conv_fwd_side(big, k3 ? 3 : 4, k3 ? 1 : 2) != small) { hulc_set_error("%s: out_side does not belong to in_side", who); return 1; }
            if (dgr && !src[k]->bits) { hulc_set_error("%s: a data-gradient job needs its mask (the ReLU bit words in bits)", who); return 1; }
            if (fwd && !src[k]->bias) { hulc_set_error("%s: a forward job needs its bias", who); return 1; }
        }
    }
    static void *dp = nullptr, *zp = nullptr;
    static int* ctr = nullptr;
    if (!dp && hipMalloc(&dp, 8192) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
    if (!zp) { if (hipMalloc(&zp, 256) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; } hipMemset(zp, 0, 256); }
    if (!ctr && hipMalloc(&ctr, 256) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
    hipMemsetAsync(ctr, 0, 256, st);      // job k claims through ctr + 16 k
    if (wgr) {
        // weight gradients: the launch writes one slab per workgroup, each job's slabs are then summed into its own output as hulc_k_conv_wgrad does.  Synchronises
        const bool c1 = stage == HULC_PAIR_CONV1_WGRAD, c3 = stage == HULC_PAIR_CONV3_WGRAD;
        const int KC = c1 ? 192 : (c3 ? 576 : 512), CO = c1 ? 32 : 64;
        float* part = nullptr;
        if (hipMalloc(&part, sizeof(float) * (size_t)(wg_a + wg_b) * CO * KC) != hipSuccess) { hulc_set_error("%s: hipMalloc failed", who); return 1; }
        const hulc_conv_job* src[2] = {a, b};
        const int wg[2] = {wg_a, wg_b};
        int ns[2] = {0, 0};
        bool okw = false;
        if (c1) {      // fp32 NCHW frames (the headline boundary): both jobs on conv1_wgrad_tr2_kernel<6, 2>
            Wgrad1Job J[2];
            for (int k = 0; k < 2; ++k) {
                Wgrad1Job q{}; q.S = Conv1Src{src[k]->in, nullptr, 0, 0}; q.work_ctr = ctr + 16 * k; q.dY = (const h16_t*)src[k]->w; q.bias_part = (float*)src[k]->bits;
                q.Nf = src[k]->frames; q.IH = q.IW = src[k]->in_side; q.OH = q.OW = src[k]->out_side;
                J[k] = q;
            }
            J[0].part = part;
            size_t l0 = 0, l1 = 0; int r, nb;
            okw = conv1_wgrad_plan(J[0].S, J[0].IH, J[0].IW, J[0].OH, J[0].OW, r, nb, l0) == conv1_wgrad_plan(J[1].S, J[1].IH, J[1].IW, J[1].OH, J[1].OW, r, nb, l1);
            if (okw) {
                for (int k = 0; k < 2; ++k) { hipMemsetAsync(src[k]->bits, 0, sizeof(float) * CO, st); hipMemsetAsync(src[k]->out, 0, sizeof(float) * CO * KC, st); }
                okw = launch_conv1_wgrad_jobs(st, J, 2, 1024, wg, ns);
            }
        } else {
            WgradJob J[2];
            for (int k = 0; k < 2; ++k) {
                WgradJob q{}; q.X = (const h16_t*)src[k]->in; q.dY = (const h16_t*)src[k]->w; q.bias_part = (float*)src[k]->bits; q.zeros = (const h16_t*)zp; q.work_ctr = ctr + 16 * k;
                q.Nf = src[k]->frames; q.IH = q.IW = src[k]->in_side; q.OH = q.OW = src[k]->out_side; q.FPB = 1;
                J[k] = q;
            }
            J[0].part = part;
            using W3 = WgradCamW<64, 3>; using W2 = WgradCamW<32, 4>;
            okw = c3 ? (a->in_side == W3::stat && b->in_side == W3::gripper) : (a->in_side == W2::stat && b->in_side == W2::gripper);      // the shapes the launch takes: nothing is written otherwise
            if (okw) {
                for (int k = 0; k < 2; ++k) { hipMemsetAsync(src[k]->bits, 0, sizeof(float) * CO, st); hipMemsetAsync(src[k]->out, 0, sizeof(float) * CO * KC, st); }
                okw = c3 ? launch_conv_wgrad_pair<64, 64, 3, 3, 1>(st, J[0], J[1], 512, wg, ns) : launch_conv_wgrad_pair<32, 64, 4, 4, 2>(st, J[0], J[1], 512, wg, ns);
            }
        }
        if (okw) {
            hipLaunchKernelGGL(unpack_conv_wgrad_kernel, dim3((CO * KC + 1023) / 1024), dim3(256), 0, st, part, ns[0], (long long)CO * KC, (float*)a->out, CO, KC, 1, 1, 0);
            hipLaunchKernelGGL(unpack_conv_wgrad_kernel, dim3((CO * KC + 1023) / 1024), dim3(256), 0, st, part + (long long)ns[0] * CO * KC, ns[1], (long long)CO * KC, (float*)b->out, CO, KC, 1, 1, 0);
        }
        const hipError_t e = hipStreamSynchronize(st);
        hipFree(part);
        if (!okw) { hulc_set_error("%s: unsupported shape (the two cameras' maps only)", who); return 1; }
        if (e != hipSuccess) { hulc_set_error("%s: %s", who, hipGetErrorString(e)); return 1; }
        if (slabs) { slabs[0] = ns[0]; slabs[1] = ns[1]; }
        return 0;
    }
    ConvTileP j[2]; int wg[2] = {wg_a, wg_b};
    const hulc_conv_job* src[2] = {a, b};
    const int n = b ? 2 : 1;
    for (int k = 0; k < n; ++k) {
        ConvTileP p{}; p.img = (const h16_t*)src[k]->in; p.IMH = p.IMW = src[k]->in_side; p.w = (const h16_t*)src[k]->w; p.out = (h16_t*)src[k]->out; p.OUTH = p.OUTW = src[k]->out_side;
        p.Nf = src[k]->frames; p.dump = (h16_t*)dp;
        if (fwd) { p.bias = src[k]->bias; p.relu = 1; p.bits_out = (unsigned*)src[k]->bits; }
        else { p.maskbits = (const unsigned*)src[k]->bits; p.zeros = (const h16_t*)zp; }
        p.work_ctr = ctr + 16 * k;
        j[k] = p;
    }
    bool ok = false;
    if (stage == HULC_PAIR_CONV2_FWD) ok = launch_conv_reg_fwd_jobs<32, 4, 4, 2>(st, j, n, wg);
    else if (stage == HULC_PAIR_CONV3_FWD) ok = launch_conv_reg_fwd_jobs<64, 3, 3, 1>(st, j, n, wg);
    else if (stage == HULC_PAIR_CONV3_DGRAD) ok = launch_conv_reg_jobs<64, 3, 3, 1, true, 1, 4, true, 1>(st, j, n, wg);
    else ok = launch_conv_reg_jobs<64, 2, 2, 1, true, 2, 4, true, 1>(st, j, n, wg);
    if (!ok) { hulc_set_error("%s: unsupported shape", who); return 1; }
    if (hipGetLastError() != hipSuccess) { hulc_set_error("%s: launch failed", who); return 1; }
    return 0;
}

// host arithmetic only: what plan_conv_reg decides for a weights-in-registers form (the modes of hulc_k_conv_tile: 10 / 11 / 17, 20 / 21 / 27, 22 / 23 / 28 / 29 and the
// bf16-only 12 / 13 / 18 / 19), a frame count, the map sides (in_side / out_side as hulc_k_conv_tile takes them) and the workgroups of the job (wgs < 1: the grid a single
// launch takes).  The geometry does not depend on the 16-bit type.  Non-zero where the form does not take the shape; no device call
int k_conv_plan(int form, int frames, int in_side, int out_side, int wgs, int* nbands, int* rows_per_band, int* frames_per_band, int* items) {
    static const char* who = "hulc_k_conv_plan";
    if (!nbands || !rows_per_band || !frames_per_band || !items || frames < 1 || in_side < 1 || out_side < 1 || in_side > 4096 || out_side > 4096) { hulc_set_error("%s: null argument or frames=%d, in_side=%d, out_side=%d out of range", who, frames, in_side, out_side); return 1; }
    const int m10 = form % 10;
    const bool known = (form >= 10 && form <= 13) || (form >= 17 && form <= 23) || (form >= 27 && form <= 29);
    if (!known) { hulc_set_error("%s: form %d is not a weights-in-registers form", who, form); return 1; }
    const bool dg = m10 == 2 || m10 == 3 || m10 == 8 || m10 == 9, k3 = m10 == 0 || m10 == 2 || m10 == 8, bitsf = m10 == 8 || m10 == 9;
    if (k_conv_fwd_side(dg ? out_side : in_side, k3 ? 3 : 4, k3 ? 1 : 2) != (dg ? in_side : out_side)) { hulc_set_error("%s: form %d: out_side %d does not belong to in_side %d", who, form, out_side, in_side); return 1; }
    const h16_t* al = reinterpret_cast<const h16_t*>((uintptr_t)0x10000);       // never dereferenced: stands for an operand that is present
    ConvTileP p{}; p.IMH = p.IMW = in_side; p.OUTH = p.OUTW = out_side; p.Nf = frames;
    if (!dg) p.relu = 1;
    else { p.zeros = al; if (bitsf) p.maskbits = reinterpret_cast<const unsigned*>(al); else p.mask = al; }
    size_t lds = 0; int it = 0; double work = 0;
    bool ok = false;
    const int w8 = wgs > 0 ? wgs : 256, w4 = wgs > 0 ? wgs : 512;
    if (form == 10) ok = plan_conv_reg<64, 3, 3, 1, false, 1, 8, true>(p, w8, lds, it, work);
    else if (form == 11 || form == 17) ok = plan_conv_reg<32, 4, 4, 2, false, 1, 8, true>(p, w8, lds, it, work);
    else if (form == 20) ok = plan_conv_reg<64, 3, 3, 1, false, 1, 4>(p, w4, lds, it, work);
    else if (form == 21 || form == 27) ok = plan_conv_reg<32, 4, 4, 2, false, 1, 4, true>(p, w4, lds, it, work);
    else if (form == 22 || form == 28) ok = plan_conv_reg<64, 3, 3, 1, true, 1, 4, true, 1>(p, w4, lds, it, work);
    else if (form == 23 || form == 29) ok = plan_conv_reg<64, 2, 2, 1, true, 2, 4, true, 1>(p, w4, lds, it, work);
    else if (form == 12 || form == 18) ok = plan_conv_reg<64, 3, 3, 1, true>(p, w8, lds, it, work);
    else ok = plan_conv_reg<64, 2, 2, 1, true, 2>(p, w8, lds, it, work);
    if (!ok) { hulc_set_error("%s: form %d does not take frames=%d, in_side=%d, out_side=%d", who, form, frames, in_side, out_side); return 1; }
    *nbands = p.FPB > 1 ? 1 : p.nbands; *rows_per_band = p.RB; *frames_per_band = p.FPB; *items = it;
    return 0;
}

}  // namespace HULC_NS
