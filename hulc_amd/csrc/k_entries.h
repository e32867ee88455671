// hulc_amd/csrc/k_entries.h — per-kernel test entries of the 16-bit encoder head and of the action loss (include/hulc_hip.h: hulc_k_spatial_softmax64,
// hulc_k_enc_tail_fwd, hulc_k_enc_tail_bwd, hulc_k_logistic_loss).  Included by engine.h inside each translation unit, so every entry exists once per
// 16-bit type (hulc_bf16 / hulc_f16; iengine.h declares them).  Nothing here restates a kernel: each entry checks its arguments, then launches through the
// helper the engine calls (enc_tail.h) or with the grid and block of the engine's launch site (engine_encoders.inc, engine_forward.inc).
#pragma once
#include "iengine.h"
#include "kernels.h"
#include "enc_tail.h"

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
    if (!dout) hipLaunchKernelGGL(spatial_softmax_fwd64_kernel, dim3(Nf), dim3(256), 0, st, (const h16_t*)f, H, W, (h16_t*)out, stats);
    else hipLaunchKernelGGL(spatial_softmax_bwd64_kernel, dim3(Nf), dim3(256), 0, st, (const h16_t*)f, (const float*)stats, dout, H, W, (h16_t*)df);
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

// T of dheads: 0 = float, 1 = this translation unit's 16-bit type
int k_logistic_loss(int t16, int wide, const float* heads, int ldh, const float* actions, const float* robot_obs, int B, int S, int nmix, int ndim, int num_classes,
                    float log_scale_min, float gripper_alpha, int gripper_control, int discrete_gripper, float grad_scale, const float* lscale, float* row_loss, float* a_tcp_out,
                    void* dheads, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    constexpr int NMIX = 10;                       // Engine::NMIX, the serial kernel's compile-time mixture count
    if (B < 1 || S < 1 || (long long)B * S > (1 << 24) || nmix != NMIX || ndim < 1 || ndim > (discrete_gripper ? 6 : 7) || num_classes < 2) {
        hulc_set_error("hulc_k_logistic_loss: B=%d S=%d nmix=%d (must be %d) ndim=%d (1..%d) num_classes=%d", B, S, nmix, NMIX, ndim, discrete_gripper ? 6 : 7, num_classes); return 1;
    }
    if (ldh < 3 * nmix * ndim + (discrete_gripper ? 2 : 0)) { hulc_set_error("hulc_k_logistic_loss: ldh=%d narrower than the heads", ldh); return 1; }
    if (!heads || !actions || !row_loss || !dheads || (gripper_control && !robot_obs)) { hulc_set_error("hulc_k_logistic_loss: null argument"); return 1; }
    const int SB = S * B;
    constexpr int ll_block = 64;                   // engine_forward.inc: one wave per workgroup
#define HULC_K_LL(TT)                                                                                                                                              \
    do {                                                                                                                                                           \
        if (wide) hipLaunchKernelGGL((logistic_loss_wide_kernel<TT>), dim3(SB), dim3(128), 0, st, heads, ldh, actions, robot_obs, B, S, nmix, ndim, num_classes,     \
                                     log_scale_min, gripper_alpha, gripper_control, grad_scale, row_loss, a_tcp_out, (TT*)dheads, discrete_gripper, lscale);         \
        else hipLaunchKernelGGL((logistic_loss_kernel<TT, NMIX>), dim3(cdiv(SB * 8, ll_block)), dim3(ll_block), 0, st, heads, ldh, actions, robot_obs, B, S, nmix,  \
                                ndim, num_classes, log_scale_min, gripper_alpha, gripper_control, grad_scale, row_loss, a_tcp_out, (TT*)dheads, discrete_gripper,    \
                                lscale);                                                                                                                           \
    } while (0)
    if (t16) HULC_K_LL(h16_t);
    else {
#ifdef HULC_HALF_F16
        hulc_set_error("hulc_k_logistic_loss: the fp32 instances live in the bf16 translation unit"); return 1;
#else
        HULC_K_LL(float);
#endif
    }
#undef HULC_K_LL
    return k_launched("hulc_k_logistic_loss");
}

}  // namespace HULC_NS
