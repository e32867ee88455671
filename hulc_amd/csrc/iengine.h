// hulc_amd/csrc/iengine.h — the interface the C-ABI (capi.hip) drives; implemented by Engine<T> (engine.h) once per compute type:
// fp32 (parity) and bf16 in capi.hip's translation unit, fp16 in engine_f16.hip (common.h explains the per-TU half format).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/hulc_hip.h"
#include "comm.h"

void hulc_set_error(const char* fmt, ...);

struct IEngine {
    virtual ~IEngine() { delete comm; delete comm_pending; }
    virtual int bind(float* p, float* g, float* m, float* v, int64_t numel, int n, const char* const* names, const int64_t* offs,
                     const int64_t* numels) = 0;
    virtual int prepare_weights(bool shadow_fresh = false) = 0;
    virtual int zero_grads() = 0;
    virtual int flush_grads() = 0;
    virtual int forward(const hulc_batch* b, float lw, float cw, float* out, int on_host) = 0;
    virtual int forward_pair(const hulc_batch* vis, const hulc_batch* lang, float lw, float cw, float* out8, int on_host) = 0;
    virtual int backward(int part = -1) = 0;   // -1: everything; 0: all but the perceptual encoders; 1: encoders (after part 0)
    virtual int validate(const hulc_batch* b, const hulc_val_noise* nz, float* out17, int32_t* plan_pp_out, int32_t* plan_pr_out, float* pred_pp_out,
                         float* pred_pr_out) = 0;
    virtual int clip_gt_encode(const float* lang_emb, int m, int slot) = 0;
    virtual int clip_gt_scores(int slot, float* out_host, int64_t cap, int32_t* n_out, int32_t* m_out) = 0;
    // ---- BC-Z / MIA language auxiliary heads (engine.h, aux_heads.h)
    virtual int aux_heads_enable(int bc_z, int mia) = 0;
    virtual int decoder_select(int decoder, int criterion) = 0;
    virtual int decoder_body_select(int body) = 0;
    virtual int aux_weights_set(float bc_z_weight, float mia_weight) = 0;
    virtual int aux_losses_get(float* out_host4) = 0;
    virtual int rollout_reset() = 0;
    virtual int rollout_plan(const hulc_rollout_obs* obs, const float* goal_static, const float* goal_gripper, const float* goal_lang,
                             const int32_t* plan_inject, int32_t* plan_out) = 0;
    virtual int rollout_act(const hulc_rollout_obs* obs, const float* u_mix, const float* u_act, float* action_out) = 0;
    virtual int rollout_get_goal(float* latent_goal_out) = 0;
    virtual int rollout_set_state(const void* plan, const float* latent_goal) = 0;
    // ---- batched multi-environment rollout (engine_rollout_envs.inc, rollout_step.h)
    virtual int rollout_envs_init(int max_envs) = 0;
    virtual int rollout_envs_reset(int n, const int32_t* slots, int clear_hidden) = 0;
    virtual int rollout_envs_plan(const hulc_rollout_envs_obs* obs, const float* goal_static, const float* goal_gripper, const float* goal_lang,
                                  const void* plan_inject, void* plan_out, float* latent_goal_out) = 0;
    virtual int rollout_envs_act(const hulc_rollout_envs_obs* obs, const float* u_mix, const float* u_act, float* actions_out) = 0;
    virtual int rollout_envs_get_state(int n, const int32_t* slots, void* plan_out, float* latent_goal_out) = 0;
    virtual int rollout_envs_set_state(int n, const int32_t* slots, const void* plan, const float* latent_goal) = 0;
    virtual int optim(const hulc_optim& o) = 0;
    int adam(float lr, float b1, float b2, float eps, int64_t step, float gscale) {
        hulc_optim o{}; o.kind = HULC_OPT_ADAM; o.lr = lr; o.beta1 = b1; o.beta2 = b2; o.eps = eps; o.step = step; o.grad_scale = gscale;
        return optim(o);
    }
    virtual int scaler_enable(float init_scale, float growth, float backoff, int interval) = 0;
    virtual int scaler_get(float* scale, int32_t* tracker, int64_t* skipped, int32_t* last_inf, int64_t* taken) = 0;
    virtual int scaler_set(float scale, int32_t tracker, int64_t taken) = 0;
    // ---- gradient clipping / gradient norms inside the optimizer step (engine.h: optim)
    virtual int grad_clip_set(int32_t algo, float limit, int32_t track) = 0;
    virtual int grad_norm_get(float* total, float* coef, float* per_tensor, int64_t cap) = 0;
    // ---- per-tensor trainable mask (engine_trainable.inc)
    virtual int trainable_set(int32_t n, const uint8_t* trainable) = 0;
    virtual int trainable_get(int64_t cap, uint8_t* trainable_out, int64_t* frozen_steps_out) = 0;
    virtual int trainable_steps_set(int32_t n, const int64_t* frozen_steps, int64_t steps_taken) = 0;
    // ---- averaged weights (engine_ema.inc)
    virtual int ema_enable(float* buf, float decay, int64_t start_step, int32_t warmup) = 0;
    virtual int ema_state_get(int64_t* updates, float* last_decay) = 0;
    virtual int ema_state_set(int64_t updates) = 0;
    virtual int ema_swap() = 0;
    virtual int ema_is_swapped(int32_t* out) = 0;
    // ---- data-parallel gradient all-reduce (comm.h): whole buffer after a finished backward, or bucketed inside the backward
    virtual int allreduce_grads(int bucket_dtype) = 0;
    virtual int backward_allreduce(int bucket_dtype) = 0;
    virtual int comm_buckets(int64_t* lo, int64_t* hi, int cap) = 0;        // the bucket ranges in issue order; returns their number
    GradComm* comm = nullptr;
    GradComm* comm_pending = nullptr;       // prepared (RCCL resolved, private stream) but not yet initialised
    int comm_prepare() {
        if (comm || comm_pending) return 0;
        GradComm* c = new GradComm();
        if (c->prepare()) { delete c; return 1; }
        comm_pending = c;
        return 0;
    }
    int comm_init(const void* unique_id, int rank, int world) {
        if (comm) { hulc_set_error("hulc_comm_init: this context already has a communicator"); return 1; }
        if (comm_prepare()) return 1;
        GradComm* c = comm_pending; comm_pending = nullptr;
        if (c->init(unique_id, rank, world)) { delete c; return 1; }
        comm = c;
        return 0;
    }
    int comm_destroy() { delete comm; comm = nullptr; delete comm_pending; comm_pending = nullptr; return 0; }
    virtual int get_tensor(const char* name, float* out, int64_t cap, int64_t* n) = 0;
    virtual int get_plan_idx(int32_t* out, int64_t cap) = 0;
    virtual int64_t workspace_bytes() const = 0;
    virtual void set_kl_beta(float b) = 0;
    virtual void set_dropout(float p) = 0;
    void set_timing(bool on, const char* filter) { timing = on; timing_filter = (filter && *filter) ? std::string(",") + filter + "," : std::string(); }
    // runtime options (hulc_set_option).  "persistent_rnn": 1 (default) = the 2048-wide recurrences of the 16-bit engines run as one
    // persistent launch each (rnn_persist.h) after a first launch has verified the XCD census on this device; 0 = one launch per time step
    // (what a process that SHARES the GPU's CUs with another process must choose: the persistent launch needs all 256 CUs resident)
    // "fused_transformer": 1 (default) = one launch per plan-recognition encoder layer in the forward of the 16-bit engines (tr_fused.h, S <= 32);
    // 0 = the seven unfused launches per layer (what the fp32 engine and S > 32 run) — tests compare the two
    // "persist_under_comm": 0 (default) = recurrences that follow an issued all-reduce bucket of hulc_backward_allreduce run one launch per step (RCCL's
    // kernels hold CUs; a persistent launch needs all of them); 1 = keep them persistent.  "comm_timing": 1 = hulc_backward_allreduce records events around
    // every bucket's collective and at the end of the backward (hulc_comm_timeline).  "debug_poison_partials": tests only — fills the weight-gradient
    // partial arena with NaN before the next backward (a slab that is read before it is written then shows up in the gradients).
    // "lazy_zero_grads": 1 (default; 16-bit engines) = hulc_zero_grads only marks the large store-first weight gradients stale instead of zeroing them
    // (engine.h: LazyG); 0 = the plain memset of the whole buffer.
    int repro_opt = 0;      // "reproducible" as last set; Engine::repro is the latched value the launches read
    int persist_mode = 1, tr_fused_mode = 1, persist_under_comm = 0, comm_timing = 0, poison_partials = 0, persist_fault = 0, lazy_zero_mode = 1, u8_fold_mode = 1, force_vote_word = 0, hold_buckets_mode = 1;
    virtual int get_option(const char* name, long long* value) = 0;
    virtual void dp_skip_vote(int phase) = 0;
    virtual void set_adam_fuse(bool on) = 0;
    int set_option(const char* name, long long value) {
        if (name && !strcmp(name, "persistent_rnn")) { persist_mode = value != 0; return 0; }
        if (name && !strcmp(name, "fused_transformer")) { tr_fused_mode = value != 0; return 0; }
        if (name && !strcmp(name, "persist_under_comm")) { persist_under_comm = value != 0; return 0; }
        // "reproducible" (default 0): every launch of the training step, the validation pass and the optimizer step sums in a fixed order — no float atomics with
        // two or more contributors per destination, no dynamic work claim under an accumulator (the audit table).  May be flipped between steps:
        // latched by the next hulc_zero_grads (no forward pending) / forward / validate.  "nondeterministic_sites" (read only): the audit's bitmask, see repro_sites.h
        if (name && !strcmp(name, "reproducible")) { repro_opt = value != 0; return 0; }
        // "dp_hold_buckets" (default 1): mcil with the tanh-RNN plan encoder under hulc_backward_allreduce — the decoder's and the plan proposal's buckets are issued BEHIND
        // the BiRNN backward so that its four recurrences stay persistent (no RCCL kernel holds CUs yet); 0 = issue them as early as possible (round 5), the BiRNN
        // backward then runs one launch per step unless persist_under_comm is set
        if (name && !strcmp(name, "dp_hold_buckets")) { hold_buckets_mode = value != 0; return 0; }
        if (name && !strcmp(name, "comm_timing")) { comm_timing = value != 0; return 0; }
        if (name && !strcmp(name, "debug_poison_partials")) { poison_partials = value != 0; return 0; }
        if (name && !strcmp(name, "lazy_zero_grads")) { lazy_zero_mode = value != 0; return 0; }
        if (name && !strcmp(name, "epilogue_fast")) { epilogue_fast = value != 0; return 0; }
        // "adam_fused_transposes" (default 1; 16-bit engines): the Adam / AdamW step writes the transposed 16-bit weight copies itself (kernels.h adam_tiled_kernel); 0 = flat pass + batched transpose
        if (name && !strcmp(name, "adam_fused_transposes")) { set_adam_fuse(value != 0); return 0; }
        if (name && !strcmp(name, "timer_event_fence")) { event_flags = value != 0 ? hipEventDefault : hipEventDisableSystemFence; for (auto& kv : timers) { for (auto& ev : kv.second.ev) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); } kv.second.ev.clear(); kv.second.used = 0; } return 0; }
        // "u8_fold": 1 (default; 16-bit engines) = the uint8 ingest path multiplies the exact byte values and applies x = u (2/255) - 1 in conv1's epilogue /
        // weight-gradient slabs (conv1_stage.h Conv1Src::fold); 0 = the value x itself is staged (16-bit rounded), as in rounds 2 - 4
        if (name && !strcmp(name, "u8_fold")) { u8_fold_mode = value != 0; return 0; }
        // "dp_skip_vote": for a gradient all-reduce done OUTSIDE the library (the torch.distributed fallback): 1 right before the collective that covers the
        // perceptual-encoder gradients, 2 right after it — the job-wide "a recurrence of this step failed on some rank" vote (engine.h skip_vote_put)
        if (name && !strcmp(name, "dp_skip_vote")) { dp_skip_vote((int)value); return 0; }
        if (name && !strcmp(name, "debug_vote_word")) { force_vote_word = value != 0; return 0; }      // tests: vote through the engine's own word even if the layout has a padding element
        if (name && !strcmp(name, "debug_persist_fault")) { persist_fault = (int)value; return 0; }      // tests: the next `value` persistent launches (after the probed first one) lose a producer
        hulc_set_error("hulc_set_option: unknown option '%s'", name ? name : "(null)");
        return 1;
    }
    hipStream_t st = nullptr;
    // ---- per-kernel-class HIP-event timers (bench.py roofline leg): events are recorded on `st` around the launches of a class
    struct KTimer { std::string name, bound; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; double flops = 0, bytes = 0; long long launches = 0; };
    std::map<std::string, KTimer> timers;
    bool epilogue_fast = true;              // hulc_set_option "epilogue_fast" 0: every GEMM epilogue through the generic path (A/B)
    bool timing = false;
    std::string timing_filter;      // empty = every class; else ",a,b,": only the listed classes (keeps event overhead out of the timed region)
    int timer_depth = 0;            // a group scope (e.g. the S recurrent steps) suppresses the per-launch scopes inside it
    unsigned event_flags = hipEventDisableSystemFence;     // hulc_set_option "timer_event_fence" 1: default events (A/B of the timers' own cost)
    struct TimerScope {
        IEngine* e; IEngine::KTimer* t;
        TimerScope(IEngine* e_, const char* name, const char* bound, double flops, double bytes, int nlaunch = 1) : e(e_), t(nullptr) {
            if (!e->timing || e->timer_depth > 0) return;
            if (!e->timing_filter.empty() && e->timing_filter.find(std::string(",") + name + ",") == std::string::npos) return;
            e->timer_depth++;
            t = &e->timers[name];
            if (t->name.empty()) { t->name = name; t->bound = bound; }
            // timing-only events: no system-scope fence when they complete (hipEventDisableSystemFence) — a default event's cache write-back + invalidate stalled the
            // stream for 5.5 us per record behind the conv kernels (profiles/r05_host_lead.txt: 20 records = 117 us of a 3.1 ms step); timers_read synchronises the stream
            if (t->used == t->ev.size()) { hipEvent_t a, b; hipEventCreateWithFlags(&a, e->event_flags); hipEventCreateWithFlags(&b, e->event_flags); t->ev.emplace_back(a, b); }
            t->flops += flops; t->bytes += bytes; t->launches += nlaunch;
            hipEventRecord(t->ev[t->used].first, e->st);
        }
        // work of a launch that is known only once the launcher has taken the shape (scope opened with 0 flops / bytes / launches)
        void add(double flops, double bytes, int nlaunch = 1) { if (t) { t->flops += flops; t->bytes += bytes; t->launches += nlaunch; } }
        ~TimerScope() { if (t) { hipEventRecord(t->ev[t->used].second, e->st); t->used++; e->timer_depth--; } }
    };
    int timers_read(char* out, int64_t cap, bool reset) {
        hipStreamSynchronize(st);
        std::string js = "{";
        bool first = true;
        for (auto& kv : timers) {
            KTimer& t = kv.second;
            double ms = 0;
            for (size_t i = 0; i < t.used; ++i) { float x = 0; hipEventElapsedTime(&x, t.ev[i].first, t.ev[i].second); ms += x; }
            char buf[512];
            snprintf(buf, sizeof(buf), "%s\"%s\": {\"bound\": \"%s\", \"launches\": %lld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}", first ? "" : ", ",
                     t.name.c_str(), t.bound.c_str(), t.launches, ms, t.flops, t.bytes);
            js += buf; first = false;
            if (reset) { t.used = 0; t.flops = t.bytes = 0; t.launches = 0; }
        }
        js += "}";
        if ((int64_t)js.size() + 1 > cap) { hulc_set_error("hulc_timers_read: buffer too small"); return 1; }
        memcpy(out, js.c_str(), js.size() + 1);
        return 0;
    }
};

// factories, one per translation unit
#define HULC_TU_DECLS                                                                                                                         \
    IEngine* make_engine(const hulc_config& cfg, int* rc);                                                                                   \
    int k_gemm_nt(int is_f32, const void* A, const void* B, float* C, int M, int N, int K, long long lda, long long ldb, long long ldc, \
                  const float* bias, int relu, void* stream);                                                                                \
    int k_spatial_softmax64(const void* f, int H, int W, int Nf, void* out, float* stats, const float* dout, void* df, void* stream);          \
    int k_enc_tail_fwd(int Nf, int ldemb, const hulc_enc_tail_job* a, const hulc_enc_tail_job* b, void* emb, const float* pos, int S,           \
                       float drop_p, unsigned long long seed, float* xf, void* xt, float* z0, float* z1, void* stream);                         \
    int k_enc_tail_bwd(int Nf, int ldemb, const hulc_enc_tail_bwd_job* a, const hulc_enc_tail_bwd_job* b, const float* demb, void* stream);     \
    int k_logistic_loss(int t16, int wide, const float* heads, int ldh, const float* actions, const float* robot_obs, int B, int S, int nmix,   \
                        int ndim, int num_classes, float log_scale_min, float gripper_alpha, int gripper_control, int discrete_gripper,         \
                        float grad_scale, const float* lscale, float* row_loss, float* a_tcp_out, void* dheads, void* stream);                  \
    int k_det_head_loss(int t16, const void* H1, const void* W, const float* bias, const float* actions, const float* robot_obs, int B, int S, int criterion,     \
                        int frame, float grad_scale, const float* lscale, float* row_loss, float* pred, float* dpre, void* stream);                              \
    int k_det_head_bwd(int t16, const float* dpre, const void* W, const void* H1, int B, int S, void* dH1, void* dZ1, float* dW, float* db, void* stream);        \
    int k_det_head_act(int t16, const void* h1, const void* W, const float* bias, const float* robot_obs, int n, float* out, void* stream);                       \
    int k_plan_kl_sample(const float* pr_logits, const float* pp_logits, int B, int NCAT, int NCLS, const int* idx_in, int* idx_out, float* probs,  \
                         float* kl_cat, float* dpp, float* dpr, float w_pp, float w_pr, unsigned long long seed, const float* lscale, void* stream); \
    int k_st_softmax_bwd(int t16, const float* probs, const float* dplan, const float* dpr_kl, const float* dpp_kl, int rows, int NCLS, float* out,  \
                         void* out_t, void* dpp_t, void* stream);                                                                               \
    int k_plan_gather(int t16, const void* w_t, const int* idx, int B, int NCAT, int NCLS, int H, const float* b1, const float* b2, float* out,   \
                      const void* emb, void* embg, int S, int W, const void* goal, int G, int grow0, void* cb, void* stream);                     \
    int k_plan_scatter_grad(int t16, int form, const void* dC, const int* idx, int B, int NCAT, int NCLS, int H, int KIN, float* dw, int store,   \
                            void* stream);                                                                                                      \
    int k_normal_kl_sample(int t16, const float* pr_state, const float* pp_state, int B, int n, const float* eps_in, float* eps_out, float* plan_f, \
                           void* plan_t, float* kl_elem, float* dpp, float* dpr, float w_pp, float w_pr, unsigned long long seed,                 \
                           const float* lscale, void* stream);                                                                                  \
    int k_normal_rsample_bwd(int t16, const float* dplan, const float* eps, const float* pr_state, const float* dpr_kl, int B, int n, void* out,  \
                             void* stream);                                                                                                     \
    int k_layernorm_fwd(int t16, const float* x, long long ldx, int rows, int n, const float* g, const float* b, void* out, long long ldo,        \
                        float* out_f32, long long ldf, float* stats, void* stream);                                                             \
    int k_layernorm_bwd(int t16, const float* dy, long long lddy, const float* x, long long ldx, const float* stats, const float* g, int rows,    \
                        int n, float* dx_f32, long long ldd, int accumulate, void* dx_t, long long ldt, float* dg, float* db, float drop_p,       \
                        unsigned long long seed, int bcast_rows, float bcast_div, int dy_parts, long long dy_part_stride, float* scratch,        \
                        void* stream);                                                                                                          \
    int k_layernorm_mean(int t16, const float* x, int B, int S, int n, const float* g, const float* b, float* stats, void* out, float* yout,      \
                         void* stream);                                                                                                         \
    int k_tr_layer_fwd(const hulc_tr_layer_job* j, int B, int S, int ln_in, float dp, void* stream);                                            \
    int k_tr_ffn_bwd(const hulc_tr_ffn_bwd_job* j, int B, int S, int bcast, float bdiv, float dp, void* stream);                                \
    int k_tr_attn_bwd(const hulc_tr_attn_bwd_job* j, int B, int S, int nparts, long long part_stride, float dp, void* stream);                  \
    int k_gemm_epi(int t16, const hulc_gemm_epi_job* j, int kernel, int* ran, void* stream);                                                    \
    int k_gemm_dual(const hulc_gemm_epi_job* jobs, int* ran, void* stream);                                                                     \
    int k_gemm_pick(int t16, int M, int N, int K, long long lda, long long ldb, int* pick, int* bk);                                            \
    int k_gemm_wgrad_nsplit(int t16, int M, int N, int K, int* nsplit, int* big);                                                               \
    int k_lin_bwd_stream(const void* dY, const void* X, long long ldx, int M, int N, int K, int nsplit, int store, float* dW, long long lddw,    \
                         float* db, float* slabs, void* stream);                                                                                \
    int k_conv_wgrad(const char* who, int typed, int which, const void* X, const void* dY, float* out, float* db_out, int Nf, int IH, int* slabs, \
                     void* stream);                                                                                                             \
    int k_conv1_wgrad_u8(const char* who, int typed, const void* X, const int* shifts, int pad, const void* dY, float* dw_out, float* db_out,   \
                         int Nf, int IH, int form, int fold, int* slabs, void* stream);                                                         \
    int k_conv_tile(const char* who, int typed, int mode, const void* img, const void* w, const float* bias, const void* mask, void* out,       \
                    unsigned* bits1_out, int Nf, int IMH, int OUTH, int relu, int wgs, void* stream);                                           \
    int k_conv_pair(const char* who, int typed, int stage, const hulc_conv_job* a, const hulc_conv_job* b, int wg_a, int wg_b, int* slabs,      \
                    void* stream);                                                                                                              \
    int k_conv_plan(int form, int frames, int in_side, int out_side, int wgs, int* nbands, int* rows_per_band, int* frames_per_band, int* items);
namespace hulc_bf16 { HULC_TU_DECLS }   // capi.hip: HULC_DTYPE_F32 / HULC_DTYPE_BF16
namespace hulc_f16 { HULC_TU_DECLS }    // engine_f16.hip: HULC_DTYPE_F16
